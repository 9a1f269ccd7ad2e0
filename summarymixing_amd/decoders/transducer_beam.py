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
from ..nnet.transducer.beam import TransducerBeamStream, beam_decode
from ..nnet.transducer.greedy import _weights, greedy_decode, greedy_start


class TransducerStreamContext:
    """What ``TransducerBeamSearcher.make_stream`` returns and ``forward_chunk`` carries from chunk to chunk: the device search of B
    slots (``search``, a TransducerBeamStream) or, for ``beam_size=1``, the greedy searcher's state and the tokens emitted so far."""

    def __init__(self, B, chunk_frames, dtype, search):
        self.B, self.chunk_frames, self.dtype, self.search = B, chunk_frames, dtype, search
        self.greedy, self.greedy_start = None, None
        self.hyps = [[] for _ in range(B)]
        self.started = [False] * B
        self.calls = 0


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
        return self._tuple(r)

    def _tuple(self, r):
        """A TransducerBeamResult -> the 4-tuple, through one host copy; the caps' warning and ``last_overflow``."""
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
                          RuntimeWarning, stacklevel=3)
        nbest_hyps = [[[int(k) for k in tokens[b, i, :int(lens[b, i])]] for i in range(int(n[b]))] for b in range(B)]
        nbest_keys = [[float(keys[b, i]) for i in range(int(n[b]))] for b in range(B)]
        best = [h[0] if h else [] for h in nbest_hyps]
        score = float(torch.tensor([k[0] if k else float("-inf") for k in nbest_keys], dtype=torch.float64).exp().mean())
        return best, score, nbest_hyps, nbest_keys

    def make_stream(self, B, chunk_frames, max_symbols, dtype=torch.float32, captured=False):
        """-> the context of B streams fed in chunks of at most chunk_frames frames (``forward_chunk``).  max_symbols: the cap on a
        hypothesis' symbols over the WHOLE stream, required (there is no T to derive it from; the searcher's own max_symbols is that
        of ``forward``).  captured=True replays one captured step (nnet.transducer.TransducerBeamStream)."""
        if int(B) != B or B < 1 or int(chunk_frames) != chunk_frames or chunk_frames < 1:
            raise ValueError(f"TransducerBeamSearcher.make_stream: B and chunk_frames must be integers >= 1, got {B}, {chunk_frames}")
        if max_symbols is None or int(max_symbols) != max_symbols or max_symbols < 1:
            raise ValueError(f"TransducerBeamSearcher.make_stream: max_symbols must be an integer >= 1, got {max_symbols}")
        if self.beam_size == 1:
            return TransducerStreamContext(int(B), int(chunk_frames), dtype, None)
        emb, dec, proj_dec = self.decode_network_lst
        search = TransducerBeamStream(emb, dec, proj_dec, self.tjoint, self.classifier_network[0], int(B), int(chunk_frames), self.beam_size,
                                      int(max_symbols), self.nbest, self.lm, self.lm_weight, self.state_beam, self.expand_beam,
                                      self.max_expansions, dtype, None, captured)
        return TransducerStreamContext(int(B), int(chunk_frames), dtype, search)

    def forward_chunk(self, tn_chunk, context, lengths=None, start=None):
        """tn_chunk (B, C, J): one chunk of the encoder output after proj_enc, for the context ``make_stream`` returned.  lengths: B host
        ints in [0, C], this chunk's frames per slot (None: all C); start: B host bools, the slots that begin a new utterance with this
        chunk (None: all on the first call, none afterwards).  -> ``forward``'s 4-tuple for the hypotheses SO FAR: what ``forward`` returns
        for the frames each slot has been given since its start, so after the last chunk the whole utterance's.  One host copy per
        chunk; the caps' warning and ``last_overflow`` as ``forward``."""
        if not isinstance(context, TransducerStreamContext):
            raise TypeError("TransducerBeamSearcher.forward_chunk: context must be what make_stream returned")
        if context.search is not None:
            return self._tuple(context.search.decode_chunk(tn_chunk, lengths, start))
        ctx, B, C = context, context.B, context.chunk_frames
        if tn_chunk.dim() != 3 or tuple(tn_chunk.shape[:2]) != (B, C) or tn_chunk.dtype != ctx.dtype:
            raise ValueError(f"TransducerBeamSearcher.forward_chunk: made for chunks ({B}, {C}, J) {ctx.dtype}, got {tuple(tn_chunk.shape)} "
                             f"{tn_chunk.dtype}")
        lengths = [C] * B if lengths is None else [int(n) for n in lengths]
        start = [ctx.calls == 0] * B if start is None else [bool(s) for s in start]
        if len(lengths) != B or len(start) != B or any(n < 0 or n > C for n in lengths):
            raise ValueError(f"TransducerBeamSearcher.forward_chunk: lengths {lengths} must be {B} integers in [0, chunk_frames = {C}] "
                             f"and start {B} booleans")
        never = [b for b in range(B) if lengths[b] > 0 and not (start[b] or ctx.started[b])]
        if never:
            raise ValueError(f"TransducerBeamSearcher.forward_chunk: frames for slots {never}, which were never started")
        emb, dec, proj_dec = self.decode_network_lst
        if ctx.greedy is None:
            ctx.greedy_start = greedy_start(B, _weights(tn_chunk, emb, dec, proj_dec, self.tjoint, self.classifier_network[0]))
            ctx.greedy = type(ctx.greedy_start)(*(t.clone() for t in ctx.greedy_start))
        for b in range(B):
            if start[b]:
                for dst, src in zip(ctx.greedy, ctx.greedy_start):
                    dst[b].copy_(src[b])
                ctx.hyps[b] = []
        ctx.started = [a or b for a, b in zip(ctx.started, start)]
        ctx.calls += 1
        rel = torch.tensor(lengths, dtype=torch.float64) / C
        r = greedy_decode(tn_chunk, emb, dec, proj_dec, self.tjoint, self.classifier_network[0], lengths=rel, state=ctx.greedy)
        ctx.greedy = r.state
        packed = torch.cat([r.tokens.float(), r.counts.view(B, 1).float(), r.scores.view(B, 1)], 1).cpu()       # the one host copy
        for b in range(B):
            ctx.hyps[b] += [int(k) for k in packed[b, :int(packed[b, C])]]
        self.last_overflow = [0] * B
        return [list(h) for h in ctx.hyps], float(packed[:, C + 1].exp().mean()), None, None
