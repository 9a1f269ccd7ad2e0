"""speechbrain.decoders.transducer.TransducerBeamSearcher as the transducer recipes instantiate it for testing (recipe key
``Beamsearcher``, …transducer.yaml:383-393: ``beam_size: 10``, ``nbest: 1``, ``lm_module: lm_model``, ``lm_weight: 0.50``,
``state_beam: 2.3``, ``expand_beam: 2.3``): beam search with the RNNLM, the whole search on the device (nnet/transducer/beam.py,
csrc/tbeam.hip) and ONE copy to the host at the end.  A recipe points its ``Beamsearcher:`` line here; ``decoders.transducer`` keeps
what it was (greedy decoding, and a refusal of everything else).  ``beam_size=1`` runs that greedy path.  No parameters of its own: it
holds the recipe's modules, as SpeechBrain's searcher does outside the checkpointed ``modules``.  SpeechBrain's source is not part of
the reference tree: the constructor arguments are the recipe's, the search and the returned 4-tuple are written from memory
(which also defines the two caps ``max_expansions`` and ``max_symbols`` upstream does not have)."""
import warnings

import torch

from ..lobes.models.RNNLM import RNNLM
from ..nnet.transducer.beam import beam_decode
from ..nnet.transducer.greedy import greedy_decode


class TransducerBeamSearcher(torch.nn.Module):
    def __init__(self, decode_network_lst, tjoint, classifier_network, blank_id, beam_size=4, nbest=5, lm_module=None, lm_weight=0.0,
                 state_beam=2.3, expand_beam=2.3, max_expansions=None, max_symbols=None):
        super().__init__()
        dn, cn = list(decode_network_lst), list(classifier_network)
        if len(dn) != 3 or len(cn) != 1:
            raise NotImplementedError("TransducerBeamSearcher: decode_network_lst = [emb, dec, proj_dec] and classifier_network = "
                                      "[transducer_lin] (the transducer recipe's) are what the kernels cover")
        if int(blank_id) != dn[0].blank_id:
            raise ValueError(f"TransducerBeamSearcher: blank_id {blank_id} differs from the embedding's {dn[0].blank_id}")
        if isinstance(beam_size, bool) or int(beam_size) != beam_size or not 1 <= beam_size <= 32:
            raise NotImplementedError(f"TransducerBeamSearcher: beam_size={beam_size} is outside [1, 32], what the selection kernel holds")
        if int(nbest) != nbest or nbest < 1 or nbest > beam_size:
            raise NotImplementedError(f"TransducerBeamSearcher: nbest={nbest} must be in [1, beam_size={beam_size}]: a frame closes with at "
                                      "most beam_size hypotheses")
        if lm_module is not None and not (isinstance(lm_module, RNNLM) and lm_module.return_hidden):
            raise NotImplementedError("TransducerBeamSearcher: lm_module must be this package's lobes.models.RNNLM.RNNLM with "
                                      f"return_hidden=True (the recipe's lm_model), got {type(lm_module).__name__}")
        if lm_weight < 0.0:
            raise ValueError(f"TransducerBeamSearcher: lm_weight must be >= 0, got {lm_weight}")
        # plain attributes, not registered submodules: the searcher adds nothing to any state_dict
        object.__setattr__(self, "decode_network_lst", dn)
        object.__setattr__(self, "classifier_network", cn)
        object.__setattr__(self, "tjoint", tjoint)
        object.__setattr__(self, "lm", lm_module)
        self.blank_id, self.beam_size, self.nbest = int(blank_id), int(beam_size), int(nbest)
        self.lm_weight, self.state_beam, self.expand_beam = float(lm_weight), float(state_beam), float(expand_beam)
        self.max_expansions, self.max_symbols = max_expansions, max_symbols
        self.last_overflow = None           # per utterance of the last call: bit 0 max_expansions ended a frame, bit 1 max_symbols was reached

    def forward(self, tn_output):
        """tn_output (B, T, J): the encoder output after proj_enc -> (best hyps: B lists of ints, exp(best keys).mean() as a float,
        nbest hyps per utterance: B lists of lists, nbest keys per utterance: B lists of floats); a key is a hypothesis' summed
        log-probability (the LM's share included) over its length counted with the leading blank.  beam_size=1: the greedy search,
        (hyps, exp(log-probability).mean(), None, None).  The tuple has no place for the caps: when an utterance hit one, its result
        may differ from upstream's, so the call warns (RuntimeWarning) and ``last_overflow`` holds the per-utterance bits."""
        emb, dec, proj_dec = self.decode_network_lst
        if self.beam_size == 1:
            r = greedy_decode(tn_output, emb, dec, proj_dec, self.tjoint, self.classifier_network[0])
            B, T = r.tokens.shape
            packed = torch.cat([r.tokens.float(), r.counts.view(B, 1).float(), r.scores.view(B, 1)], 1).cpu()    # the one host copy
            hyps = [[int(k) for k in packed[b, :int(packed[b, T])]] for b in range(B)]
            self.last_overflow = [0] * B
            return hyps, float(packed[:, T + 1].exp().mean()), None, None
        r = beam_decode(tn_output, emb, dec, proj_dec, self.tjoint, self.classifier_network[0], self.beam_size, self.nbest, self.lm,
                        self.lm_weight, self.state_beam, self.expand_beam, None, self.max_expansions, self.max_symbols)
        B, nb, U = r.tokens.shape
        packed = torch.cat([r.tokens.reshape(B, nb * U).double(), r.lengths.double(), r.scores.double(), r.n_hyps.view(B, 1).double(),
                            r.overflow.view(B, 1).double()], 1).cpu()
        tokens, lens = packed[:, :nb * U].long().view(B, nb, U), packed[:, nb * U:nb * U + nb].long()       # the one host copy, taken apart
        keys, n = packed[:, nb * U + nb:nb * U + 2 * nb], packed[:, nb * U + 2 * nb].long()
        self.last_overflow = [int(v) for v in packed[:, nb * U + 2 * nb + 1]]
        if any(self.last_overflow):
            hit = [b for b, v in enumerate(self.last_overflow) if v]
            warnings.warn(f"TransducerBeamSearcher: utterances {hit} hit max_expansions (bit 0) or max_symbols (bit 1), overflow = "
                          f"{[self.last_overflow[b] for b in hit]}: their result may differ from an unbounded search's (last_overflow)",
                          RuntimeWarning, stacklevel=2)
        nbest_hyps = [[[int(k) for k in tokens[b, i, :int(lens[b, i])]] for i in range(int(n[b]))] for b in range(B)]
        nbest_keys = [[float(keys[b, i]) for i in range(int(n[b]))] for b in range(B)]
        best = [h[0] if h else [] for h in nbest_hyps]
        score = float(torch.tensor([k[0] if k else float("-inf") for k in nbest_keys], dtype=torch.float64).exp().mean())
        return best, score, nbest_hyps, nbest_keys
