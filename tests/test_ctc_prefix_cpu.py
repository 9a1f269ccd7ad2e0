"""CTC prefix scoring without a GPU: the float64 restatement of DESIGN.md §I.23 (tests/_ctc_prefix_ref.py) against brute force over
every alignment, the descriptor of csrc/ctc_prefix.hip against include/smx.h, what the three entries refuse before any launch, and
every refusal of decoders.scorer and of S2SBeamSearcher's scorer argument by its message."""
import ctypes
import itertools
import math

import pytest
import torch

from tests import _ctc_prefix_ref as P

EINVAL = -1
_BASE = 1 << 40


def _collapse(path, blank):
    out, prev = [], None
    for k in path:
        if k != prev and k != blank:
            out.append(k)
        prev = k
    return out


@pytest.mark.parametrize("T,V,blank", [(1, 3, 0), (2, 3, 0), (3, 4, 3), (4, 3, 1), (5, 3, 0), (5, 4, 3)])
def test_restatement_equals_brute_force_over_every_alignment(T, V, blank):
    """exp(psi(g)) = the summed probability of every alignment whose collapsed labelling starts with g; the eos column = the full CTC
    probability of g; along chains of extensions that include a repeated token and a prefix longer than T (probability 0)."""
    x = torch.log_softmax(torch.randn(T, V, dtype=torch.float64, generator=torch.Generator().manual_seed(7 * T + V)), -1)
    eos = V                                                   # outside the vocabulary: no column is special but blank
    labels = [k for k in range(V) if k != blank]
    starts, exact = {}, {}
    for path in itertools.product(range(V), repeat=T):
        p = math.exp(sum(float(x[t, k]) for t, k in enumerate(path)))
        lab = _collapse(path, blank)
        exact[tuple(lab)] = exact.get(tuple(lab), 0.0) + p
        for n in range(len(lab) + 1):
            starts[tuple(lab[:n])] = starts.get(tuple(lab[:n]), 0.0) + p
    assert abs(starts[()] - 1.0) < 1e-12
    checked = 0
    for g in itertools.chain.from_iterable(itertools.product(labels, repeat=n) for n in range(0, 4)):
        state, last = P.empty(x, T, blank), None
        for c in g:
            state, last = P.extend(x, T, blank, state, last, c), c
        want = starts.get(tuple(g), 0.0)
        assert abs(math.exp(float(state[2])) - want) < 1e-12, (g, "psi")
        # the columns: psi(g c) - psi(g) for every c, the blank column, and an eos column placed on each label in turn
        ctc, p1 = P.scores(x, T, blank, eos, state, last)
        assert float(ctc[blank]) == P.NEG_INF and not torch.isnan(ctc).any()
        for c in labels:
            assert abs(math.exp(float(p1[c])) - starts.get(tuple(g) + (c,), 0.0)) < 1e-12, (g, c)
            if want > 0.0:
                assert abs(math.exp(float(ctc[c])) * want - starts.get(tuple(g) + (c,), 0.0)) < 1e-12
            nxt = P.extend(x, T, blank, state, last, c)
            assert float(nxt[2]) == float(p1[c]) or abs(float(nxt[2]) - float(p1[c])) < 1e-12, "extend and scores agree on psi'"
        e = labels[0]
        _, pe = P.scores(x, T, blank, e, state, last)
        assert abs(math.exp(float(pe[e])) - exact.get(tuple(g), 0.0)) < 1e-12, (g, "the eos column is the whole sequence")
        if want == 0.0:
            assert float(state[2]) == P.NEG_INF and bool((ctc == P.NEG_INF).all()), "a prefix no alignment reaches scores -inf, never NaN"
        checked += 1
    assert checked == 1 + len(labels) + len(labels) ** 2 + len(labels) ** 3


def test_descriptor_size_and_offsets_match_header():
    from summarymixing_amd import _lib
    A = _lib.CtcPrefixArgs
    assert ctypes.sizeof(A) == 160
    assert A.x.offset == 0 and A.ldx.offset == 8 and A.enc_len.offset == 16 and A.score.offset == 24 and A.done.offset == 32
    assert A.n_tok.offset == 40 and A.tokens.offset == 48 and A.anc.offset == 56 and A.state.offset == 64 and A.psi.offset == 72
    assert A.logits.offset == 80 and A.ldz.offset == 88 and A.extra.offset == 96 and A.lde.offset == 104 and A.inv_temp.offset == 112
    assert A.weight.offset == 120 and A.dtype.offset == 124 and A.B.offset == 128 and A.T.offset == 140 and A.eos.offset == 152
    assert ctypes.sizeof(_lib.S2SBeamArgs) == 296, "smx_s2s_beam_args is what it was"


def test_entries_refuse_null_pointers_and_bad_sizes():
    """Refused on the host before any launch (the pointers are fake and never dereferenced)."""
    from summarymixing_amd import _lib
    lib = _lib.lib()
    ptrs = [n for n, t in _lib.CtcPrefixArgs._fields_ if t is ctypes.c_void_p]
    needs = {"init": {"x", "enc_len", "state", "psi"},
             "advance": {"x", "enc_len", "state", "psi", "score", "done", "n_tok", "tokens", "anc"},
             "score": set(ptrs) - {"anc"}}

    def call(entry, **kw):
        a = _lib.CtcPrefixArgs(ldx=40, ldz=40, lde=40, inv_temp=1.0, weight=0.4, dtype=0, B=2, W=3, V=40, T=70, cap=8, blank=0, eos=2,
                               **{n: _BASE + i * 0x100000 for i, n in enumerate(ptrs)})
        for k, v in kw.items():
            setattr(a, k, v)
        return getattr(lib, f"smx_ctc_prefix_{entry}")(ctypes.byref(a), None)
    for entry in needs:
        assert getattr(lib, f"smx_ctc_prefix_{entry}")(None, None) == EINVAL
        for kw in (dict(B=0), dict(W=0), dict(V=0), dict(T=0), dict(cap=0), dict(T=4097), dict(ldx=39), dict(blank=-1), dict(blank=40),
                   dict(eos=-1), dict(eos=0), dict(B=1 << 20, W=128)):
            assert call(entry, **kw) == EINVAL, (entry, kw)
        for n in needs[entry]:
            assert call(entry, **{n: None}) == EINVAL, (entry, n)
    assert call("score", T=4097) == EINVAL and b"4096" in lib.smx_last_error()
    for kw in (dict(dtype=2), dict(ldz=39), dict(lde=39), dict(weight=0.0), dict(weight=1.5), dict(weight=float("nan")), dict(inv_temp=0.0),
               dict(inv_temp=float("inf"))):
        assert call("score", **kw) == EINVAL, kw


class _Lin:                                                   # what a CTCScorer asks of its head: .w.weight / .w.bias
    def __init__(self, V=5, d=4):
        self.w = torch.nn.Linear(d, V)


_RECIPE = dict(bos_index=1, eos_index=2, min_decode_ratio=0.0, max_decode_ratio=1.0, using_eos_threshold=False, length_normalization=True)


def test_scorer_classes_take_the_recipes_arguments_and_refuse_by_name():
    from summarymixing_amd import decoders
    from summarymixing_amd.decoders.scorer import CTCScorer, ScorerBuilder, active
    assert decoders.scorer.CTCScorer is CTCScorer and decoders.ScorerBuilder is ScorerBuilder
    lin = _Lin()
    ctc = CTCScorer(eos_index=2, blank_index=0, ctc_fc=lin)
    assert (ctc.eos_index, ctc.blank_index, ctc.ctc_fc, ctc.ctc_window_size) == (2, 0, lin, 0)
    with pytest.raises(NotImplementedError, match="ctc_window_size=20"):
        CTCScorer(eos_index=2, blank_index=0, ctc_fc=lin, ctc_window_size=20)
    with pytest.raises(TypeError, match="ctc_fc"):
        CTCScorer(eos_index=2, blank_index=0, ctc_fc=object())
    with pytest.raises(ValueError, match="distinct"):
        CTCScorer(eos_index=2, blank_index=2, ctc_fc=lin)
    b = ScorerBuilder(full_scorers=[ctc], weights={"ctc": 0.4})
    assert b.ctc is ctc and b.ctc_weight == 0.4 and active(b) is b
    b = ScorerBuilder(full_scorers=[ctc], weights={"ctc": 0.3}, scorer_beam_scale=0.3)          # CommonVoice
    assert b.ctc_weight == 0.3 and b.scorer_beam_scale == 0.3
    assert active(ScorerBuilder(full_scorers=[ctc], weights={"ctc": 0.0})) is None and active(None) is None
    with pytest.raises(NotImplementedError, match="partial_scorers"):
        ScorerBuilder(full_scorers=[ctc], partial_scorers=[ctc], weights={"ctc": 0.4})
    with pytest.raises(NotImplementedError, match="Linear in full_scorers"):
        ScorerBuilder(full_scorers=[torch.nn.Linear(2, 2), ctc], weights={"ctc": 0.4})
    with pytest.raises(NotImplementedError, match="'transformerlm'"):
        ScorerBuilder(full_scorers=[ctc], weights={"ctc": 0.4, "transformerlm": 0.6})
    with pytest.raises(NotImplementedError, match="exactly one CTCScorer, got 2"):
        ScorerBuilder(full_scorers=[ctc, ctc], weights={"ctc": 0.4})
    with pytest.raises(NotImplementedError, match="exactly one CTCScorer, got 0"):
        ScorerBuilder(weights={"ctc": 0.4})
    with pytest.raises(ValueError, match="under 'ctc'"):
        ScorerBuilder(full_scorers=[ctc])
    for w in (-0.1, 1.5):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            ScorerBuilder(full_scorers=[ctc], weights={"ctc": w})
    with pytest.raises(NotImplementedError, match="ScorerBuilder, got object"):
        active(object())


def test_beam_searcher_takes_a_builder_and_adds_nothing_to_any_state_dict():
    from summarymixing_amd.decoders import CTCScorer, S2SBeamSearcher, ScorerBuilder
    model, lin, head = torch.nn.Linear(4, 4), torch.nn.Linear(4, 3), _Lin()
    b = ScorerBuilder(full_scorers=[CTCScorer(eos_index=2, blank_index=0, ctc_fc=head)], weights={"ctc": 0.4})
    s = S2SBeamSearcher(modules=[model, lin], beam_size=10, scorer=b, **_RECIPE)
    assert s.scorer is b and len(s.state_dict()) == 0 and list(s.parameters()) == [] and list(s.children()) == []
    assert S2SBeamSearcher(modules=[model, lin], beam_size=10, **_RECIPE).scorer is None
    with pytest.raises(NotImplementedError, match="scorer must be a decoders.scorer.ScorerBuilder"):
        S2SBeamSearcher(modules=[model, lin], beam_size=10, scorer=object(), **_RECIPE)
    with pytest.raises(NotImplementedError, match="got CTCScorer"):
        S2SBeamSearcher(modules=[model, lin], beam_size=10, scorer=b.ctc, **_RECIPE)
