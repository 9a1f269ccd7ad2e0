"""speechbrain.nnet.embedding.Embedding as the transducer recipe instantiates it for the prediction network (``emb``,
…transducer.yaml:301-304: ``consider_as_one_hot: True``): token k becomes the one-hot row of width ``num_embeddings - 1`` with the
blank's column removed, the blank itself a zero row.  The module keeps SpeechBrain's frozen ``Embedding.weight`` table
(num_embeddings, num_embeddings - 1), so reference checkpoints load unchanged; the forward writes the rows with a HIP kernel from
the tokens alone.  GPU only.  (SpeechBrain's source is not part of the reference tree: the table layout below was written from
memory of SpeechBrain 1.0 - see DESIGN.md §I.10.)"""
import torch
from torch import nn

from .. import ops


class Embedding(nn.Module):
    def __init__(self, num_embeddings, embedding_dim=128, consider_as_one_hot=False, blank_id=0):
        super().__init__()
        if not consider_as_one_hot:
            raise NotImplementedError("a trainable Embedding is not used by the SummaryMixing recipes (consider_as_one_hot=True only)")
        if not 0 <= int(blank_id) < int(num_embeddings) or num_embeddings < 2:
            raise ValueError(f"Embedding: blank_id {blank_id} outside the vocabulary of {num_embeddings}")
        self.num_embeddings = int(num_embeddings)
        self.consider_as_one_hot = True
        self.embedding_dim = self.num_embeddings - 1
        self.blank_id = int(blank_id)
        # rows below the blank: e_k; the blank: zeros (padding_idx); rows above it: e_{k-1}
        self.Embedding = nn.Embedding(self.num_embeddings, self.embedding_dim, padding_idx=self.blank_id)
        one_hot = torch.eye(self.embedding_dim)
        with torch.no_grad():
            self.Embedding.weight.zero_()
            self.Embedding.weight[:self.blank_id] = one_hot[:self.blank_id]
            self.Embedding.weight[self.blank_id + 1:] = one_hot[self.blank_id:]
        self.Embedding.weight.requires_grad = False

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("summarymixing_amd kernels run on the GPU only (no CPU fallback)")
        return ops.onehot_rows(x, self.num_embeddings, self.blank_id, self.Embedding.weight.dtype)
