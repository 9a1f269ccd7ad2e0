"""The transducer's prediction network in one call: tokens -> one-hot input product -> LSTM -> dropout -> ``proj_dec``
(…transducer.yaml:291-310 and the recipe's ``dec_emb_dropout`` / ``dec_dropout``).  No one-hot row is written: the input product
is a row gather of W_ih^T, its weight gradient a deterministic scatter (csrc/lstm.hip)."""
import torch

from ... import functional as F
from ... import ops
from ..embedding import Embedding
from ..linear import Linear
from ..RNN import LSTM, lstm_apply


def _seeds(emb_dropout, dec_dropout, training):
    """One seed per active dropout site, the embedding's first: the order prediction_network_masks replays."""
    s_emb = ops.new_dropout_seed() if (training and emb_dropout > 0.0) else None
    s_dec = ops.new_dropout_seed() if (training and dec_dropout > 0.0) else None
    return s_emb, s_dec


def prediction_network_masks(B, U1, H, emb_dropout, dec_dropout, device):
    """The masks the NEXT training-mode prediction_network call with these rates draws, as fp32 factors (0 or 1 / (1 - p)):
    (keep (B, U1) per token | None, hmask (B, U1, H) on the LSTM output | None).  Draws the same seeds from the same stream
    (ops.new_dropout_seed), so a test pins ops._drop_state["counter"] before this call and again before the call it checks."""
    s_emb, s_dec = _seeds(emb_dropout, dec_dropout, True)
    keep = ops.token_keep(B * U1, emb_dropout, s_emb, device).view(B, U1) if s_emb is not None else None
    hmask = None
    if s_dec is not None:
        hmask = ops.dropout(torch.ones((B * U1, H), dtype=torch.float32, device=device), dec_dropout, s_dec).view(B, U1, H)
    return keep, hmask


def prediction_network(tokens_bos, emb, dec, proj_dec, emb_dropout=0.0, dec_dropout=0.0, training=False, hx=None):
    """proj_dec(dropout(dec(dropout(emb(tokens_bos)))[0])) -> (B, U+1, J), ready for Tjoint / transducer_joint_loss, in the dtype of
    emb's table.  tokens_bos (B, U+1) integer; emb an Embedding(consider_as_one_hot=True), dec an LSTM, proj_dec a Linear of this
    package.  Elementwise dropout of a one-hot row only matters at its hot element, so emb_dropout is ONE Bernoulli keep per token
    scaled 1 / (1 - p): the same distribution as the recipe's; dec_dropout is the library's counter-based dropout on h.  Same value
    and gradients as the drop-in chain (bit for bit without dropout; dW_ih and db_ih up to the order of their fp32 sums)."""
    if not (isinstance(emb, Embedding) and isinstance(dec, LSTM) and isinstance(proj_dec, Linear)):
        raise TypeError("prediction_network: emb, dec and proj_dec must be this package's Embedding, LSTM and Linear")
    if not tokens_bos.is_cuda:
        raise RuntimeError(ops.NO_CPU)
    if tokens_bos.dim() != 2 or tokens_bos.dtype.is_floating_point:
        raise ValueError(f"prediction_network: integer tokens (B, U+1) expected, got {tuple(tokens_bos.shape)} {tokens_bos.dtype}")
    if dec.rnn.input_size != emb.embedding_dim:
        raise ValueError(f"prediction_network: dec takes {dec.rnn.input_size} features, emb gives {emb.embedding_dim}")
    if not (0.0 <= emb_dropout < 1.0 and 0.0 <= dec_dropout < 1.0):
        raise ValueError("prediction_network: dropout rates must be in [0, 1)")
    B, U1 = tokens_bos.shape
    H = dec.hidden_size
    dtype = emb.Embedding.weight.dtype
    s_emb, s_dec = _seeds(emb_dropout, dec_dropout, training)
    keep = ops.token_keep(B * U1, emb_dropout, s_emb, tokens_bos.device) if s_emb is not None else None
    h, _, _ = lstm_apply(tokens_bos, hx, dec, onehot=(emb.num_embeddings, emb.blank_id, keep, dtype))
    if s_dec is not None:
        def run(xin, need_bwd):
            y = ops.dropout(xin.reshape(B * U1, H), dec_dropout, s_dec).view(B, U1, H)
            if not need_bwd:
                return y, None
            return y, lambda dy: ops.dropout(dy.reshape(B * U1, H).contiguous(), dec_dropout, s_dec).view(B, U1, H)
        h = F.block(h, run, [])
    return proj_dec(h)
