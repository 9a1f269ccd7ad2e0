"""smx_lm_score (csrc/lm_score.hip) on the GPU against float64 (tests/_transformerlm_ref.lm_score), through the C-ABI so
that the leading dimensions and the alignment of the rows are the test's: V in {5, 37, 40, 5003} (fewer columns than lanes, a tail of
V % 4 / V % 8, whole groups only, more than one ROW_DEPTH sweep of a lane), F32 and BF16 logits, temperatures 1.0 and 1.15, both
accumulate modes, rows 16-byte aligned and not - the same bits.  Bar: 4 x the error of weight * torch.log_softmax(z.float() / T) in
float32 on the GPU against float64 (8 eps of the largest value where ATen is exact).  R = 16 rows, B = 4 utterances of W = 4:
  row 1 dead (score -inf), row 2 holds a NaN, row 3 is all -inf, row 4 has one -inf column, row 6 has a NaN score;
  utterance 2 is done, utterance 3 sits at n_tok == cap.
Rows that score nothing write -inf when accumulate == 0 and are left alone when accumulate == 1; a NaN / no-number row is -inf in
both.  The floats around and between the rows of extra keep their sentinel; two runs agree bit for bit."""
import ctypes

import pytest
import torch

from tests import _transformerlm_ref as LR
from tests._util import report

pytestmark = pytest.mark.gpu
B, W, CAP, WEIGHT = 4, 4, 9, 0.6
R = B * W
NEG = float("-inf")
SENTINEL = 12345.0
GUARD = 64


def _inputs(V, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(R, V, generator=g) * 3.0).to(dtype)
    z[2, V // 2] = float("nan")
    z[3] = NEG
    z[4, V - 1] = NEG
    extra0 = torch.randn(R, V, generator=g)
    extra0[5, 0] = NEG                                        # -inf in extra stays -inf
    extra0[0, V - 1] = NEG
    score = torch.randn(R, generator=g)
    score[1] = NEG
    score[6] = float("nan")
    done = torch.tensor([0, 0, 1, 0], dtype=torch.uint8)
    n_tok = torch.tensor([0, 3, 5, CAP], dtype=torch.int32)
    return z, extra0, score, done, n_tok


def _strided(t, ld, off, fill):
    """t (R, V) inside a flat buffer: GUARD + off floats, then R rows of leading dimension ld, then GUARD -> (buffer, view)."""
    Rr, V = t.shape
    buf = torch.full((GUARD + off + Rr * ld + GUARD,), fill, dtype=t.dtype)
    view = buf[GUARD + off:GUARD + off + Rr * ld].view(Rr, ld)[:, :V]
    view.copy_(t)
    buf = buf.cuda()
    return buf, buf[GUARD + off:GUARD + off + Rr * ld].view(Rr, ld)[:, :V]


def _run(z, extra0, score, done, n_tok, temp, acc, aligned):
    from summarymixing_amd import _lib as L
    V = z.shape[1]
    ld, off = ((V + 7) // 8 * 8, 0) if aligned else (V + 1 + (V % 2), 1)      # unaligned: an odd leading dimension from an odd offset
    zb, zv = _strided(z, ld, off, 0.0)
    eb, ev = _strided(extra0, ld, off, SENTINEL)
    assert aligned == all((zv[r].data_ptr() % 16 == 0 and ev[r].data_ptr() % 16 == 0) for r in range(R))
    sc, dn, nt = score.cuda(), done.cuda(), n_tok.cuda()
    a = L.LmScoreArgs(logits=zv.data_ptr(), ldz=ld, extra=ev.data_ptr(), lde=ld, score=sc.data_ptr(), done=dn.data_ptr(), n_tok=nt.data_ptr(),
                      inv_temp=1.0 / temp, weight=WEIGHT, dtype=L.BF16 if z.dtype == torch.bfloat16 else L.F32, B=B, W=W, V=V, cap=CAP,
                      accumulate=acc)
    L.check(L.lib().smx_lm_score(ctypes.byref(a), torch.cuda.current_stream().cuda_stream), "smx_lm_score")
    torch.cuda.synchronize()
    out = ev.cpu().clone()
    guard = eb.cpu().clone()
    body = guard[GUARD + off:GUARD + off + R * ld].view(R, ld)
    assert bool((guard[:GUARD + off] == SENTINEL).all()) and bool((guard[GUARD + off + R * ld:] == SENTINEL).all()), "the guard band around extra"
    assert bool((body[:, V:] == SENTINEL).all()), "the floats between the rows of extra"
    return out


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("temp", [1.0, 1.15])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("V", [5, 37, 40, 5003])
def test_lm_score_against_float64_in_both_modes_and_alignments(V, dt, temp):
    dtype = {"f32": torch.float32, "bf16": torch.bfloat16}[dt]
    z, extra0, score, done, n_tok = _inputs(V, dtype, 100 + V)
    lm64 = LR.lm_score(z.float(), temp, WEIGHT)
    aten = (WEIGHT * torch.log_softmax(z.float().cuda() / temp, -1)).cpu()
    nothing = [1, 6, 8, 9, 10, 11, 12, 13, 14, 15]           # dead, NaN score, done utterance, n_tok == cap
    no_number = [2, 3]
    ok = [r for r in range(R) if r not in nothing + no_number]
    for acc in (0, 1):
        out = _run(z, extra0, score, done, n_tok, temp, acc, True)
        assert _bits(out, _run(z, extra0, score, done, n_tok, temp, acc, False)), "aligned and unaligned rows give the same bits"
        assert _bits(out, _run(z, extra0, score, done, n_tok, temp, acc, True)), "two runs agree bit for bit"
        assert bool((out[no_number] == NEG).all()), "a row holding a NaN or no number scores -inf in both modes"
        if acc:
            assert _bits(out[nothing], extra0[nothing]), "rows that score nothing are left as they are"
            ref = extra0[ok].double() + lm64[ok]
            base = extra0[ok] + aten[ok]
        else:
            assert bool((out[nothing] == NEG).all()), "rows that score nothing write -inf"
            ref, base = lm64[ok], aten[ok]
        fin = torch.isfinite(ref)
        assert torch.equal(torch.isfinite(out[ok]), fin) and bool((out[ok][~fin] == NEG).all()), "-inf stays -inf, nothing else is"
        assert not fin[ok.index(4), V - 1] and (not acc or not fin[ok.index(5), 0])
        ours = float((out[ok].double() - ref)[fin].abs().max())
        theirs = float((base.double() - ref)[fin].abs().max())
        bar = 4.0 * theirs if theirs > 0.0 else 8.0 * torch.finfo(torch.float32).eps * float(ref[fin].abs().max())
        print(f"lm_score V {V} {dt} T {temp} acc {acc}: ours {ours:.2e}, ATen float32 {theirs:.2e}, bar {bar:.2e}")
        report(f"lm_score V{V} {dt} T{temp} acc{acc}", {"errors": {"extra": {"ours": ours, "aten": theirs, "bar": bar}}})
        assert ours <= bar
