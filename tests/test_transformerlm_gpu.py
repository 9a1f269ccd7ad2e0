"""TransformerLM (lobes.models.transformer.TransformerLM) on the GPU, on the three models of tests/_lm_models.py, in
float32 and bfloat16, against the float64 restatement of tests/_transformerlm_ref.py.  The bar is the project's: at most 4 x the error
of the ATen chain at the same dtype against float64 (tests/_decoder_ref.judge), every error report()ed.

a. forward on (B, U) = (3, 13), one row holding two pad tokens (masked as keys).
b. step, position by position for 13 steps over pad-free prefixes: within the same bar of forward's float64 logits at every position,
   and the bits of the row run alone in a state of its own: a row depends on neither R nor the other rows.
c. with an ancestor table in which the rows swap parents at steps 3, 7 and 8: the bits of a host loop that reorders the caches
   physically before each step and runs the plain step.
d. a state reset and used for a second sequence, then reset again, gives the first run's bits."""
import functools

import pytest
import torch

from tests import _decoder_ref as DR
from tests import _lm_models as LM

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
B, U, SEED = 3, 13, 3


@functools.lru_cache(maxsize=None)
def _model(name, dt):
    return LM.build(name, DT[dt], SEED)


def _tokens(seed, rows=B, pads=False):
    t = torch.randint(1, LM.V, (rows, U), generator=torch.Generator().manual_seed(seed))
    if pads:
        t[1, 4] = t[1, 9] = 0
    return t


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _run_steps(m, tokens, dtype, state=None, anc=None):
    """tokens (R, U) on the CPU through U cached steps -> (logits (R, U, V) on the CPU, the state)."""
    R = tokens.shape[0]
    st = m.make_state(R, U, dtype, "cuda") if state is None else state
    tk = tokens.to(torch.int32).cuda()
    out = [m.step(tk[:, u].contiguous(), st, anc=anc).clone() for u in range(U)]
    return torch.stack(out, 1).cpu(), st


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(LM.MODELS))
def test_forward_against_float64_with_a_padded_row(name, dt):
    m, tokens = _model(name, dt), _tokens(21, pads=True)
    with torch.no_grad():
        ours = m(tokens.cuda(), dtype=DT[dt])
    assert ours.dtype == DT[dt] and tuple(ours.shape) == (B, U, LM.V)
    ref = LM.restated(name, m, "f64", DT[dt])(tokens)
    aten = LM.restated(name, m, "aten", DT[dt])(tokens)
    assert float((ref[1, 4:] - LM.restated(name, m, "f64", DT[dt])(tokens, mask_pad=False)[1, 4:]).abs().max()) > 1e-3, "the mask matters"
    DR.judge(f"transformerlm forward {name} {dt}", DT[dt], {"logits": ours}, {"logits": aten}, {"logits": ref})


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(LM.MODELS))
def test_step_equals_forward_of_the_prefix_and_a_row_alone(name, dt):
    m, tokens = _model(name, dt), _tokens(22)
    with torch.no_grad():
        ours, _ = _run_steps(m, tokens, DT[dt])
        ref = LM.restated(name, m, "f64", DT[dt])(tokens)        # causal: position u of the whole sequence is forward(prefix)[:, -1]
        aten = LM.restated(name, m, "aten", DT[dt])(tokens)
        DR.judge(f"transformerlm step {name} {dt}", DT[dt], {"logits": ours}, {"logits": aten}, {"logits": ref})
        for b in range(B):
            alone, _ = _run_steps(m, tokens[b:b + 1], DT[dt])
            assert _bits(alone, ours[b:b + 1]), f"row {b} alone differs from row {b} among {B}"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["lm-d128-h2-pre", "lm-d768-h12-post"])
def test_ancestor_table_equals_physically_reordered_caches(name, dt):
    m, R = _model(name, dt), 4
    tokens = _tokens(23, rows=R)
    parents = {3: [1, 0, 3, 2], 7: [2, 2, 0, 1], 8: [3, 0, 0, 2]}       # step -> the row of step - 1 each row continues
    with torch.no_grad():
        st_a, st_p = m.make_state(R, U, DT[dt], "cuda"), m.make_state(R, U, DT[dt], "cuda")
        anc = torch.full((R, U), -1, dtype=torch.int32)
        anc_dev = anc.cuda()
        tk = tokens.to(torch.int32).cuda()
        for u in range(U):
            par = parents.get(u, list(range(R)))
            if u > 0:
                new = anc.clone()
                for r in range(R):
                    new[r, :u - 1] = anc[par[r], :u - 1]
                    new[r, u - 1] = par[r]                   # the key of position u - 1 sits in the parent's cache row
                anc = new
                anc_dev.copy_(anc)
                idx = torch.tensor(par).cuda()
                for kv in st_p.self_kv:                      # the host loop: the caches follow the hypotheses
                    kv.copy_(kv.index_select(0, idx))
            za = m.step(tk[:, u].contiguous(), st_a, anc=anc_dev)
            zp = m.step(tk[:, u].contiguous(), st_p)
            assert _bits(za, zp), f"step {u}"
        assert anc[0].tolist() != [0] * (U - 1) + [-1], "the table is not the trivial one"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_a_reused_state_gives_the_first_runs_bits(dt):
    name = "lm-d768-h12-post"
    m = _model(name, dt)
    first, other = _tokens(24), _tokens(25)
    with torch.no_grad():
        want, st = _run_steps(m, first, DT[dt])
        st.reset()
        got_other, _ = _run_steps(m, other, DT[dt], state=st)
        assert not _bits(got_other, want)
        st.reset()
        again, _ = _run_steps(m, first, DT[dt], state=st)
        assert _bits(again, want)
        assert int(st.pos.min()) == U and int(st.done.sum()) == 0
