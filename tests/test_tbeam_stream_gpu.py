"""The transducer beam search carried across streaming chunks on the GPU (smx_tbeam_resume / smx_tbeam_select_stream behind
nnet.transducer.TransducerBeamStream and TransducerBeamSearcher.forward_chunk).

The contract is chunked == whole, bit for bit: after every chunk a slot's result is torch.equal, on every field, to beam_decode over the
frames delivered so far - beam_decode being the search tests/test_tbeam_gpu.py already holds to the float64 restatement.  Both sides
always get the same explicit max_symbols = 2 T + 8 of the whole utterance.  The cases are those of tests/_tbeam_ref.py, the smallest at
which both frame exits, an expand_beam pruning, exact ties, a zero-length row and a row that ends mid-chunk occur."""
import warnings

import pytest
import torch

from tests import _greedy_ref as G
from tests import _tbeam_ref as R
from tests.test_tbeam_gpu import _assert_equals_search, _host, _mods, _setup

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
FIELDS = ("tokens", "lengths", "scores", "sums", "n_hyps", "overflow", "expansions", "frames")


def _whole(name, use_lm, dtype=F32, rows=None, n=None):
    """beam_decode over the first n frames of a case's rows (lengths cut to n) with the whole utterance's max_symbols."""
    from summarymixing_amd.nnet.transducer import beam_decode
    mods, lm, enc, lengths, W, _ = _setup(name, use_lm, dtype)
    U = 2 * enc.shape[1] + 8
    if rows is not None:
        enc, lengths = enc[rows], lengths[rows]
    if n is not None:
        enc, lengths = enc[:, :n], lengths.clamp(max=n)
    return beam_decode(enc, *mods, W, nbest=W, lm=lm, lm_weight=R.LM_WEIGHT, state_beam=R.STATE_BEAM, expand_beam=R.EXPAND_BEAM, lengths=lengths,
                       max_symbols=U)


def _stream(name, use_lm, dtype, B, C, captured=False):
    from summarymixing_amd.nnet.transducer import TransducerBeamStream
    mods, lm, enc, _, W, _ = _setup(name, use_lm, dtype)
    return TransducerBeamStream(*mods, B, C, W, 2 * enc.shape[1] + 8, nbest=W, lm=lm, lm_weight=R.LM_WEIGHT, state_beam=R.STATE_BEAM,
                                expand_beam=R.EXPAND_BEAM, dtype=dtype, captured=captured)


def _chunk(enc, at, n, C, fill=0.0):
    """(B, C, J): frames [at, at + n) of enc, the rows beyond them filled."""
    out = torch.full((enc.shape[0], C, enc.shape[2]), fill, dtype=enc.dtype, device=enc.device)
    out[:, :n] = enc[:, at:at + n]
    return out


def _lockstep(s, enc, lengths, C, fill=0.0, **kw):
    """Feed every slot its own utterance from call 0 on, C frames per call -> [(frames fed so far, result clone)] after every call."""
    out, T = [], enc.shape[1]
    for at in range(0, T, C):
        n = min(C, T - at)
        r = s.decode_chunk(_chunk(enc, at, n, C, fill), [min(max(int(l) - at, 0), C) for l in lengths], **kw)
        out.append((at + n, type(r)(*(t.clone() for t in r))))
    return out


def _assert_same(got, want, what):
    for k, g, w in zip(FIELDS, got, want):
        assert torch.equal(g, w), f"{what}: {k} differs\n{g}\n{w}"


def _row(r, b):
    return type(r)(*(t[b:b + 1] for t in r))


# ---- 1. chunked == whole
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("use_lm", [False, True], ids=["nolm", "lm"])
@pytest.mark.parametrize("name", ["small", "blank7", "tie"])
def test_chunked_equals_whole_bit_for_bit(name, use_lm, dtype):
    _, _, enc, lengths, _, _ = _setup(name, use_lm, dtype)
    B, T, _ = enc.shape
    want = _whole(name, use_lm, dtype)
    for C in (1, 5, T):
        got = _lockstep(_stream(name, use_lm, dtype, B, C), enc, lengths.tolist(), C)
        _assert_same(got[-1][1], want, f"{name} lm={use_lm} {dtype} C={C}")


# ---- 2. every pause is a whole search of the prefix
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("use_lm", [False, True], ids=["nolm", "lm"])
def test_every_pause_is_the_whole_search_of_the_prefix(use_lm, dtype):
    _, _, enc, lengths, W, _ = _setup("small", use_lm, dtype)
    got = _lockstep(_stream("small", use_lm, dtype, 3, 5), enc, lengths.tolist(), 5)
    assert [n for n, _ in got] == [5, 10, 12]
    for n, r in got:
        _assert_same(r, _whole("small", use_lm, dtype, n=n), f"small lm={use_lm} {dtype} after {n} frames")
    if dtype == F32:
        final = _host(got[-1][1])
        for b, ref in enumerate(R.reference("small", use_lm)):
            assert int(final.n_hyps[b]) == min(len(ref["hyps"]), W)
            _assert_equals_search(final, b, ref, W, f"small lm={use_lm} streamed")


# ---- 3. irregular feeding
@pytest.mark.parametrize("use_lm", [False, True], ids=["nolm", "lm"])
def test_irregular_feeding_equals_the_whole_search(use_lm):
    _, _, enc, _, _, _ = _setup("blank7", use_lm)
    s, at = _stream("blank7", use_lm, F32, 1, 8), 0
    for n in (3, 0, 5, 1, 0, 7):
        before = type(s.state.result())(*(t.clone() for t in s.state.result()))
        r = s.decode_chunk(_chunk(enc[:1], at, n, 8, float("nan")), [n])
        at += n
        if n == 0 and at > 0:
            _assert_same(r, before, "a chunk without frames")
        if at:
            _assert_same(r, _whole("blank7", use_lm, rows=[0], n=at), f"after {at} frames")
    assert at == enc.shape[1]


# ---- 4. slots: independent streams that start, sit out and start again on their own
@pytest.mark.parametrize("use_lm", [False, True], ids=["nolm", "lm"])
def test_slots_carry_independent_streams(use_lm):
    _, _, enc, _, _, _ = _setup("blank7", use_lm)
    C = 8
    u = [_whole("blank7", use_lm, rows=[b]) for b in (0, 1)]
    s = _stream("blank7", use_lm, F32, 3, C)
    blocks = lambda: s.state.state.view(3, -1).clone()
    clone = lambda r: type(r)(*(t.clone() for t in r))

    def call(parts, start):
        """parts: per slot (utterance, first frame) or None (no frames in this call)."""
        x = torch.full((3, C, enc.shape[2]), float("nan"), device="cuda")
        for b, part in enumerate(parts):
            if part is not None:
                x[b] = enc[part[0], part[1]:part[1] + C]
        return clone(s.decode_chunk(x, [0 if p is None else C for p in parts], start))

    call([(0, 0), None, (1, 0)], [True, False, True])
    r1, st1 = call([(0, 8), (1, 0), None], [False, True, False]), blocks()
    _assert_same(_row(r1, 0), u[0], "slot 0 after its last chunk")
    _assert_same(_row(r1, 2), _whole("blank7", use_lm, rows=[1], n=8), "slot 2 paused after 8 frames")
    r2, st2 = call([None, (1, 8), None], [False, False, False]), blocks()
    _assert_same(_row(r2, 1), u[1], "slot 1, started one call late")
    for b in (0, 2):                                     # slot 0 after its end and slot 2 mid-stream sat this call out
        _assert_same(_row(r2, b), _row(r1, b), f"slot {b} sat out")
        assert torch.equal(st2[b], st1[b]), f"slot {b} sat out: its state block changed"
    r3 = call([None, None, (1, 8)], [False, False, False])
    _assert_same(_row(r3, 2), u[1], "slot 2 after sitting out one call")
    call([None, None, (0, 0)], [False, False, True])
    r5 = call([None, None, (0, 8)], [False, False, False])
    _assert_same(_row(r5, 2), u[0], "slot 2, started again with a second utterance")
    _assert_same(_row(r5, 0), u[0], "slot 0, untouched since its end")


# ---- 5. the caps
def test_cap_case_in_chunks_equals_the_whole_capped_search():
    from summarymixing_amd.nnet.transducer import TransducerBeamStream, beam_decode
    Bc, T, V, H, J, blank, W, seed, E, U = R.CAP
    p, enc = G.make_case(Bc, T, V, H, J, blank, seed)
    mods, enc = _mods(p, blank), enc.cuda()
    want = beam_decode(enc, *mods, W, nbest=W, max_expansions=E, max_symbols=U)
    assert want.overflow.tolist() == [3, 3]
    s = TransducerBeamStream(*mods, Bc, 4, W, U, nbest=W, max_expansions=E)
    got = _lockstep(s, enc, [T] * Bc, 4)
    _assert_same(got[-1][1], want, "CAP at C=4")
    _assert_same(got[0][1], beam_decode(enc[:, :4], *mods, W, nbest=W, max_expansions=E, max_symbols=U), "CAP after 4 frames")


# ---- 6. a dead slot
def test_dead_slot_keeps_its_result_until_started_again():
    """Frame 3 holds NaN: the search ends there on a row without numbers (overflow bit 2, no hypothesis) - also when a pause has
    written a result before.  Further frames change nothing; a start revives the slot."""
    from summarymixing_amd.nnet.transducer import beam_decode
    mods, _, enc, _, W, _ = _setup("blank7", False)
    bad = enc[:1].clone()
    bad[0, 3] = float("nan")
    U = 2 * enc.shape[1] + 8
    want = beam_decode(bad, *mods, W, nbest=W, max_symbols=U)
    assert int(want.overflow[0]) & 4 and int(want.n_hyps[0]) == 0 and int(want.frames[0]) == 4
    s = _stream("blank7", False, F32, 1, 2)
    r0 = s.decode_chunk(bad[:, 0:2])
    assert int(r0.n_hyps[0]) >= 1                        # a pause wrote a result: the dead end must clear it
    r1 = type(r0)(*(t.clone() for t in s.decode_chunk(bad[:, 2:4])))
    _assert_same(r1, want, "the chunk with the NaN frame")
    block = s.state.state.clone()
    r2 = s.decode_chunk(bad[:, 4:6])
    _assert_same(r2, r1, "a chunk after the end")
    assert torch.equal(s.state.state, block) and int(s.state.done[0]) == 1
    got = _lockstep(s, enc[:1], [enc.shape[1]], 2, start=None)       # (start=None after the first call starts nobody: still dead)
    _assert_same(got[-1][1], r1, "still dead")
    for at in range(0, enc.shape[1], 2):
        r = s.decode_chunk(enc[:1, at:at + 2], start=[at == 0])
    _assert_same(r, _whole("blank7", False, rows=[0]), "started again")


# ---- 7. rows at and beyond lengths[b] are not read, and nothing is written outside the buffers
@torch.no_grad()
def test_unread_rows_and_poisoned_guards():
    _, lm, enc, lengths, _, _ = _setup("small", True)
    plain = _lockstep(_stream("small", True, F32, 3, 5), enc, lengths.tolist(), 5, fill=0.0)
    s = _stream("small", True, F32, 3, 5)
    st, G_, guarded = s.state, 64, {}
    for name in ("h_in", "c_in", "h_out", "c_out", "pdec", "z", "cur_tok", "lm_h_in", "lm_c_in", "state", "done", "overflow", "expansions", "frames",
                 "stream_frames", "start", "lengths", "tokens", "out_len", "scores", "sums", "n_hyps"):
        t = getattr(st, name)
        big = torch.empty(t.numel() + 2 * G_, dtype=t.dtype, device=t.device)
        big.view(torch.uint8).fill_(0xA5)
        inner = big[G_:G_ + t.numel()].view(t.shape)
        inner.copy_(t)
        setattr(st, name, inner)
        guarded[name] = (big, t.numel())
    poisoned = _lockstep(s, enc, lengths.tolist(), 5, fill=float("nan"))
    for (n, a), (_, b) in zip(plain, poisoned):
        _assert_same(b, a, f"NaN beyond lengths, after {n} frames")
    for name, (big, n) in guarded.items():
        raw, es = big.view(torch.uint8), big.element_size()
        assert bool((raw[:G_ * es] == 0xA5).all()) and bool((raw[(G_ + n) * es:] == 0xA5).all()), f"{name}: a guard was written"


# ---- 8. captured, polling, reproducibility, independence of B
@pytest.mark.parametrize("use_lm", [False, True], ids=["nolm", "lm"])
def test_captured_equals_eager_on_two_inputs(use_lm):
    _, _, enc, lengths, _, _ = _setup("small", use_lm)
    cap = _stream("small", use_lm, F32, 3, 5, captured=True)
    finals = []
    for x, l in ((enc, lengths.tolist()), (enc.flip(0).contiguous(), lengths.flip(0).tolist())):
        eager = _lockstep(_stream("small", use_lm, F32, 3, 5), x, l, 5)
        for i, at in enumerate((0, 5, 10)):                  # the one captured stream serves both inputs: every slot starts again at frame 0
            got = cap.decode_chunk(_chunk(x, at, min(5, 12 - at), 5), [min(max(n - at, 0), 5) for n in l], start=[at == 0] * 3)
            _assert_same(got, eager[i][1], f"captured, lm={use_lm}, after {at + 5} frames")
        finals.append(got.tokens.clone())
    assert not torch.equal(finals[0], finals[1])


@pytest.mark.parametrize("use_lm", [False, True], ids=["nolm", "lm"])
def test_polling_runs_and_batch_do_not_matter(use_lm):
    _, _, enc, lengths, _, _ = _setup("small", use_lm)
    lens = lengths.tolist()
    first = _lockstep(_stream("small", use_lm, F32, 3, 5), enc, lens, 5)
    again = _lockstep(_stream("small", use_lm, F32, 3, 5), enc, lens, 5)
    every = _lockstep(_stream("small", use_lm, F32, 3, 5), enc, lens, 5, poll_every=1)
    for (n, a), (_, b), (_, c) in zip(first, again, every):
        _assert_same(b, a, f"a second run, after {n} frames")
        _assert_same(c, a, f"poll_every=1, after {n} frames")
    for b in range(3):
        one = _lockstep(_stream("small", use_lm, F32, 1, 5), enc[b:b + 1], lens[b:b + 1], 5)
        for (n, a), (_, o) in zip(first, one):
            _assert_same(o, _row(a, b), f"slot {b} alone, after {n} frames")


# ---- 9. the module
def _searcher(name, use_lm, **kw):
    from summarymixing_amd.decoders.transducer_beam import TransducerBeamSearcher
    mods, lm, enc, _, W, (_, _, blank, _, _, _) = _setup(name, use_lm)
    emb, dec, proj, tj, lin = mods
    args = dict(beam_size=W, nbest=3, lm_module=lm, lm_weight=R.LM_WEIGHT if use_lm else 0.0, state_beam=R.STATE_BEAM, expand_beam=R.EXPAND_BEAM,
                max_symbols=2 * enc.shape[1] + 8)
    args.update(kw)
    return TransducerBeamSearcher([emb, dec, proj], tj, [lin], blank, **args), enc


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_forward_chunk_ends_at_forwards_tuple(captured):
    s, enc = _searcher("blank7", True)
    want = s(enc)
    ctx = s.make_stream(2, 5, s.max_symbols, captured=captured)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        for at in range(0, 16, 5):
            n = min(5, 16 - at)
            got = s.forward_chunk(_chunk(enc, at, n, 5, float("nan")), ctx, [n, n])
    assert got == want and s.last_overflow == [0, 0]


def test_forward_chunk_beam_one_equals_forwards_greedy_result():
    s, enc = _searcher("blank7", False, beam_size=1, nbest=1)
    want = s(enc)
    ctx = s.make_stream(2, 5, 40)
    for at in range(0, 16, 5):
        n = min(5, 16 - at)
        got = s.forward_chunk(_chunk(enc, at, n, 5, float("nan")), ctx, [n, n])
    assert got == want and got[2] is None and got[3] is None
    again = s.forward_chunk(_chunk(enc, 0, 5, 5), ctx, [5, 0], start=[True, False])     # slot 0 begins anew, slot 1 keeps its tokens
    assert again[0][1] == want[0][1] and again[0][0] == want[0][0][:len(again[0][0])]


def test_forward_chunk_reports_the_caps():
    from summarymixing_amd.decoders.transducer_beam import TransducerBeamSearcher
    Bc, T, V, H, J, blank, W, seed, E, U = R.CAP
    p, enc = G.make_case(Bc, T, V, H, J, blank, seed)
    emb, dec, proj, tj, lin = _mods(p, blank)
    s = TransducerBeamSearcher([emb, dec, proj], tj, [lin], blank, beam_size=W, nbest=1, max_expansions=E, max_symbols=U)
    ctx, enc = s.make_stream(Bc, 4, U), enc.cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for at in range(0, T - 4, 4):
            s.forward_chunk(enc[:, at:at + 4], ctx)
    with pytest.warns(RuntimeWarning, match="max_expansions"):
        hyps, _, _, _ = s.forward_chunk(enc[:, T - 4:], ctx)
    assert s.last_overflow == [3, 3] and hyps == [R.search(p, enc[b].cpu(), blank, W, None, E=E, U=U)["hyps"][0][0] for b in range(Bc)]
