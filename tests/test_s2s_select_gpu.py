"""smx_s2s_select and smx_s2s_embed_step (csrc/attn_step.hip) alone, through ops.

The token must equal the arg-max of the very logits tensor the kernel read: exact checks, no tolerance.  Scores and per-token
log-probabilities are held to float64 log_softmax(z / T) of the same stored logits within 4 x the error torch.log_softmax makes at
float32 on them (8 eps(float32) x the largest |log-probability| only where torch's error is exactly 0).  The embedding step is compared row by
row with tests/_decoder_ref.embed at float64 under tests/test_tgt_embed_gpu.py's bar: the ATen chain (F.embedding * sqrt(d) + pe, cast
to the dtype) beside ours, ours <= 4 x ATen's, floor 8 eps(dtype)."""

import pytest
import torch

from tests import _decoder_ref as DR
from tests._util import report

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
EPS32 = torch.finfo(torch.float32).eps


def _state(B, cap, n0=0):
    dev = "cuda"
    return dict(tok=torch.full((B,), -7, dtype=torch.int32, device=dev), done=torch.zeros(B, dtype=torch.uint8, device=dev),
                n_tok=torch.full((B,), n0, dtype=torch.int32, device=dev), score=torch.zeros(B, device=dev),
                tokens=torch.full((B, cap), -1, dtype=torch.int32, device=dev), logp_tok=torch.zeros((B, cap), device=dev))


def _select(z, st, eos, **kw):
    from summarymixing_amd import ops
    ops.s2s_select(z, st["tok"], st["done"], st["n_tok"], st["score"], st["tokens"], st["logp_tok"], eos, **kw)


def _lp_bar(z, T):
    """-> (float64 log_softmax(z / T), the bar as tests/_decoder_ref.judge sets it: 4 x the error torch.log_softmax makes at float32
    on the same logits, or 8 eps(float32) x the largest |log-probability| where torch is exact)."""
    ref = torch.log_softmax(z.double().cpu() / T, -1)
    aten = torch.log_softmax(z.float() / T, -1).double().cpu()
    err = float((aten - ref).abs().max())
    return ref, (4.0 * err if err > 0.0 else 8.0 * EPS32 * float(ref.abs().max()))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("V", [2, 63, 64, 65, 1000, 5000])
def test_token_is_the_argmax_of_the_stored_logits(V, dt):
    dtype = DT[dt]
    B, cap = 5, 4
    g = torch.Generator().manual_seed(V)
    for T in (1.0, 1.15):
        z = (torch.randn(B, V, generator=g) * 3).to(dtype).cuda()
        z[1, V // 2] = z[1].max() + 1                         # ties: the same maximum twice, the lower index wins
        z[1, V - 1] = z[1, V // 2]
        st = _state(B, cap)
        _select(z, st, eos=V + 5, inv_temp=1.0 / T)
        torch.cuda.synchronize()
        cols = torch.arange(V, device="cuda").expand_as(z)        # the lowest index of the row maximum (bfloat16 logits do tie)
        want = torch.where(z == z.max(-1, keepdim=True).values, cols, V).min(-1).values.to(torch.int32)
        assert int(want[1]) == V // 2
        assert torch.equal(st["tok"], want) and torch.equal(st["tokens"][:, 0], want) and bool((st["tokens"][:, 1:] == -1).all())
        assert bool((st["n_tok"] == 1).all()) and bool((st["done"] == 0).all())
        ref, bar = _lp_bar(z, T)
        lp_ref = ref.gather(1, want.cpu().long()[:, None])[:, 0]
        err = float((st["logp_tok"][:, 0].double().cpu() - lp_ref).abs().max())
        print(f"select V {V} {dt} T {T}: lp err {err:.2e}, bar (4 x aten) {bar:.2e}")
        report(f"s2s_select V{V} {dt} T{T}", {"errors": {"lp": {"ours": err, "bar": bar}}})
        assert err <= bar
        assert torch.equal(st["score"], st["logp_tok"][:, 0]), "score = 0 + lp"


def test_nan_column_never_wins_and_poisons_the_log_probability():
    B, V, cap = 3, 130, 2
    z = torch.randn(B, V, generator=torch.Generator().manual_seed(1)).cuda()
    z[0, 7] = float("nan")
    z[2] = float("nan")
    st = _state(B, cap)
    _select(z, st, eos=V + 1)
    zz = z.clone()
    zz[0, 7] = float("-inf")
    assert int(st["tok"][0]) == int(torch.argmax(zz[0])) and int(st["tok"][1]) == int(torch.argmax(z[1])) and int(st["tok"][2]) == -1
    lp = st["logp_tok"][:, 0]
    assert bool(torch.isnan(lp[0])) and bool(torch.isfinite(lp[1])) and bool(torch.isnan(lp[2]))


def test_eos_is_excluded_below_min_steps_and_ends_a_row_after():
    B, V, cap, eos = 4, 65, 6, 9
    z = torch.randn(B, V, generator=torch.Generator().manual_seed(2)).cuda()
    z[:, eos] = 50.0                                          # eos is the maximum everywhere
    st = _state(B, cap)
    st["n_tok"].copy_(torch.tensor([0, 1, 2, 3]))
    _select(z, st, eos, min_steps=2)
    z2 = z.clone()
    z2[:, eos] = float("-inf")
    second = torch.argmax(z2, -1).to(torch.int32)
    assert torch.equal(st["tok"][:2], second[:2]) and bool((st["tok"][2:] == eos).all())
    assert torch.equal(st["done"].cpu(), torch.tensor([0, 0, 1, 1], dtype=torch.uint8))
    assert torch.equal(st["n_tok"].cpu(), torch.tensor([1, 2, 3, 4], dtype=torch.int32))
    # the log-probability is the chosen token's under the FULL softmax (eos included in the normaliser)
    ref, bar = _lp_bar(z, 1.0)
    errs = [abs(float(st["logp_tok"][b, b]) - float(ref[b, int(st["tok"][b])])) for b in range(B)]      # (row b appended at n = b)
    print(f"select eos / min_steps: lp err {max(errs):.2e}, bar (4 x aten) {bar:.2e}")
    report("s2s_select eos min_steps", {"errors": {"lp": {"ours": max(errs), "bar": bar}}})
    assert max(errs) <= bar


def test_forced_tokens_done_rows_and_the_capacity():
    B, V, cap, eos = 4, 1000, 3, 5
    g = torch.Generator().manual_seed(3)
    z = torch.randn(B, V, generator=g).cuda()
    forced = torch.tensor([17, eos, 999, 0], dtype=torch.int32).cuda()
    st = _state(B, cap)
    st["n_tok"].copy_(torch.tensor([0, 1, 2, 1]))
    st["done"][3] = 1                                         # a finished row: nothing of it may change
    st["score"].copy_(torch.tensor([0.5, -1.0, 2.0, 3.25]))
    before = {k: v.clone() for k, v in st.items()}
    _select(z, st, eos, forced=forced)
    ref, bar = _lp_bar(z, 1.0)
    errs = [abs(float(st["logp_tok"][b, b]) - float(ref[b, int(forced[b])])) for b in range(3)]
    print(f"select forced: lp err {max(errs):.2e}, bar (4 x aten) {bar:.2e}")
    report("s2s_select forced", {"errors": {"lp": {"ours": max(errs), "bar": bar}}})
    assert max(errs) <= bar
    for b, n in ((0, 0), (1, 1), (2, 2)):
        assert int(st["tokens"][b, n]) == int(forced[b]) == int(st["tok"][b])
        lp = float(st["logp_tok"][b, n])
        assert float(st["score"][b]) == float(torch.tensor(float(before["score"][b])) + torch.tensor(lp)), "score += lp in float32"
    assert torch.equal(st["done"].cpu(), torch.tensor([0, 1, 1, 1], dtype=torch.uint8)), "eos ends row 1, n_tok == cap ends row 2"
    assert torch.equal(st["n_tok"].cpu(), torch.tensor([1, 2, 3, 1], dtype=torch.int32))
    for k in st:
        assert torch.equal(st[k][3].view(-1).view(torch.uint8), before[k][3].view(-1).view(torch.uint8)), f"done row changed {k}"
    # a second call: rows 1, 2, 3 are done and keep every bit; row 0 goes on
    mid = {k: v.clone() for k, v in st.items()}
    _select(z, st, eos, forced=forced)
    for k in st:
        assert torch.equal(st[k][1:].contiguous().view(-1).view(torch.uint8), mid[k][1:].contiguous().view(-1).view(torch.uint8)), k
    assert int(st["n_tok"][0]) == 2 and int(st["tokens"][0, 1]) == 17
    # strided logits (a row stride larger than V) and a forced token outside the vocabulary
    wide = torch.randn(B, V + 23, generator=g).cuda()
    st2 = _state(B, cap)
    _select(wide[:, :V], st2, eos=V + 1)
    assert torch.equal(st2["tok"], torch.argmax(wide[:, :V], -1).to(torch.int32))
    st3 = _state(B, cap)
    _select(z, st3, eos, forced=torch.tensor([V, -1, 3, 4], dtype=torch.int32).cuda())
    assert bool(torch.isinf(st3["logp_tok"][:2, 0]).all()) and bool(torch.isfinite(st3["logp_tok"][2:, 0]).all())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("d", [64, 512])
def test_embed_step_reads_the_row_of_the_device_counter_and_advances_it(d, dt):
    from summarymixing_amd import ops
    dtype = DT[dt]
    V, max_pos = 40, 50
    g = torch.Generator().manual_seed(d)
    table = torch.randn(V, d, generator=g).cuda()
    pe = torch.randn(max_pos + 3, d, generator=g).cuda()      # rows at and beyond max_pos exist here so a wrong read would show
    pos0 = [0, 1, max_pos - 1, max_pos, 7, 3]
    toks = [5, 39, 0, 11, V + 2, 9]                           # row 4: a token outside the vocabulary reads as a zero row
    B = len(pos0)
    tok = torch.tensor(toks, dtype=torch.int32).cuda()
    pos = torch.tensor(pos0, dtype=torch.int32).cuda()
    done = torch.zeros(B, dtype=torch.uint8).cuda()
    done[5] = 1                                               # a finished row is embedded but not advanced
    y = ops.s2s_embed_step(tok, table, pe, pos, done, max_pos, out_dtype=dtype)
    assert y.dtype == dtype and tuple(y.shape) == (B, d)
    assert pos.tolist() == [1, 2, max_pos, max_pos, 8, 3]
    assert done.tolist() == [0, 0, 0, 1, 0, 1], "the row at max_pos is marked done, not advanced"
    ours, aten, ref = {}, {}, {}
    zero = torch.zeros(1, d)
    for b in range(B):
        p = pos0[b]
        row = pe[p:p + 1].cpu() if p < max_pos else zero      # at max_pos no positional row is read: the embedding alone
        t = torch.tensor([[toks[b]]])
        key = f"row {b} pos {p}"
        ours[key] = y[b]
        aten[key] = DR.embed(t.cuda(), table, row.cuda())[0, 0].to(dtype).float()
        ref[key] = DR.embed(t, table.double().cpu(), row.double())[0, 0]
    DR.judge(f"s2s_embed_step d{d} {dt}", dtype, ours, aten, ref)
    # without a positional table
    pos2 = torch.zeros(B, dtype=torch.int32).cuda()
    y2 = ops.s2s_embed_step(tok, table, None, pos2, torch.zeros(B, dtype=torch.uint8).cuda(), max_pos, out_dtype=torch.float32)
    want = DR.embed(tok.cpu().long()[:, None], table.double().cpu(), torch.zeros(1, d, dtype=torch.float64))[:, 0]
    got = DR.embed(tok.long()[:, None], table, zero.cuda())[:, 0]
    DR.judge(f"s2s_embed_step d{d} {dt} no table", torch.float32, {"y": y2}, {"y": got}, {"y": want})
    assert pos2.tolist() == [1] * B
