"""speechbrain.decoders.transducer.TransducerBeamSearcher as the transducer recipe instantiates it for validation (recipe key
``Greedysearcher``, …transducer.yaml:375-381: ``beam_size: 1``): greedy decoding, at most one symbol per frame, with the frame loop
on the device (nnet/transducer/greedy.py, csrc/greedy.hip) and ONE copy to the host at the end.  Beam search (``beam_size > 1``,
the recipe's ``Beamsearcher``) and an ``lm_module`` are not built.  No parameters of its own: it holds the recipe's modules, as
SpeechBrain's searcher does outside the checkpointed ``modules``.  SpeechBrain's source is not part of the reference tree: the
constructor arguments are the recipe's, the returned 4-tuple and its score are written from memory."""
import torch

from ..nnet.transducer.greedy import greedy_decode


class TransducerBeamSearcher(torch.nn.Module):
    def __init__(self, decode_network_lst, tjoint, classifier_network, blank_id, beam_size=4, nbest=5, lm_module=None, lm_weight=0.0,
                 state_beam=2.3, expand_beam=2.3):
        super().__init__()
        if lm_module is not None:
            raise NotImplementedError("TransducerBeamSearcher: an lm_module belongs to beam search, which is not built "
                                      "(greedy decoding, beam_size=1, is)")
        if beam_size != 1:
            raise NotImplementedError(f"TransducerBeamSearcher: beam search (beam_size={beam_size}) is not built; "
                                      "beam_size=1 runs greedy decoding")
        dn, cn = list(decode_network_lst), list(classifier_network)
        if len(dn) != 3 or len(cn) != 1:
            raise NotImplementedError("TransducerBeamSearcher: decode_network_lst = [emb, dec, proj_dec] and classifier_network = "
                                      "[transducer_lin] (the transducer recipe's) are what the kernels cover")
        if int(blank_id) != dn[0].blank_id:
            raise ValueError(f"TransducerBeamSearcher: blank_id {blank_id} differs from the embedding's {dn[0].blank_id}")
        # plain attributes, not registered submodules: the searcher adds nothing to any state_dict
        object.__setattr__(self, "decode_network_lst", dn)
        object.__setattr__(self, "classifier_network", cn)
        object.__setattr__(self, "tjoint", tjoint)
        self.blank_id, self.beam_size, self.nbest = int(blank_id), 1, nbest
        self.lm, self.lm_weight, self.state_beam, self.expand_beam = None, lm_weight, state_beam, expand_beam

    def forward(self, tn_output):
        """tn_output (B, T, J): the encoder output after proj_enc -> (hyps: B lists of ints, score, None, None); score =
        exp(log-probability of each row's hypothesis).mean(), a float."""
        emb, dec, proj_dec = self.decode_network_lst
        r = greedy_decode(tn_output, emb, dec, proj_dec, self.tjoint, self.classifier_network[0])
        B, T = r.tokens.shape
        packed = torch.cat([r.tokens.float(), r.counts.view(B, 1).float(), r.scores.view(B, 1)], 1).cpu()    # the one host copy
        hyps = [[int(k) for k in packed[b, :int(packed[b, T])]] for b in range(B)]
        return hyps, float(packed[:, T + 1].exp().mean()), None, None
