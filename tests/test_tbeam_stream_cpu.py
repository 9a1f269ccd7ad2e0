"""The transducer beam search carried across streaming chunks, the part that needs no GPU: the float64 restatement of
the chunked search (tests/_tbeam_stream_ref.py, its own loop with a pause and a resume) against the whole search of tests/_tbeam_ref.py
on every prefix, the C-ABI's two new entries and their host-side refusals, and the refusals of the Python surface."""
import ctypes
import types

import pytest
import torch

from tests import _tbeam_ref as R
from tests import _tbeam_stream_ref as S


def _sizes(T, C):
    return [min(C, T - at) for at in range(0, T, C)]


@pytest.mark.parametrize("use_lm", [False, True], ids=["nolm", "lm"])
@pytest.mark.parametrize("name", ["small", "blank7", "tie"])
def test_chunked_restatement_equals_the_whole_search_on_every_prefix(name, use_lm):
    """After every chunk, for chunk sizes 1, 5 and T: hypotheses (tokens, sums, keys - float64, so equal means equal), their order, the
    counts, the frame exits and the overflow of _tbeam_ref.search over the frames delivered so far, with the whole utterance's U."""
    p, enc, blank, W, lm, lengths = R.case(name, use_lm)
    T = enc.shape[1]
    U = 2 * T + 8
    whole = {}
    for b in range(enc.shape[0]):
        n_b = lengths[b]
        for C in (1, 5, T):
            st = S.Stream(p, blank, W, lm, U=U)
            fed = S.feed_in_chunks(st, enc[b, :n_b], _sizes(n_b, C)) if n_b else [(0, st.feed(enc[b, :0]))]
            for n, got in fed:
                if (b, n) not in whole:
                    whole[(b, n)] = R.search(p, enc[b], blank, W, lm, n_frames=n, U=U)
                want = whole[(b, n)]
                for k in ("hyps", "overflow", "expansions", "frames", "exits"):
                    assert got[k] == want[k], (name, use_lm, b, C, n, k)
            assert fed[-1][0] == n_b
    if name == "small":
        assert whole[(1, 0)]["hyps"] == [([], 0.0, 0.0)]
        assert any(x == "state" for (b, n), w in whole.items() for x in w["exits"]) and any(x == "count" for (b, n), w in whole.items() for x in w["exits"])


def test_chunked_restatement_under_the_caps_and_fed_irregularly():
    """The CAP configuration in chunks of 4, and zero-frame chunks in the middle of a stream."""
    from tests import _greedy_ref as G
    Bc, T, V, H, J, blank, W, seed, E, U = R.CAP
    p, enc = G.make_case(Bc, T, V, H, J, blank, seed)
    for b in range(Bc):
        st = S.Stream(p, blank, W, None, E=E, U=U)
        for n, got in S.feed_in_chunks(st, enc[b], _sizes(T, 4)):
            want = R.search(p, enc[b], blank, W, None, E=E, U=U, n_frames=n)
            assert all(got[k] == want[k] for k in ("hyps", "overflow", "expansions", "frames", "exits")), (b, n)
        assert got["overflow"] == 3
    p, enc, blank, W, lm, _ = R.case("blank7", True)
    U = 2 * enc.shape[1] + 8
    st = S.Stream(p, blank, W, lm, U=U)
    fed = S.feed_in_chunks(st, enc[0], (3, 0, 5, 1, 0, 7))
    assert fed[1][1] == fed[0][1] and fed[4][1] == fed[3][1]
    want = R.search(p, enc[0], blank, W, lm, U=U)
    assert all(fed[-1][1][k] == want[k] for k in ("hyps", "overflow", "expansions", "frames", "exits"))


def test_abi_exports_bindings_and_host_side_refusals():
    from summarymixing_amd import _lib
    A = _lib.TbeamArgs
    assert ctypes.sizeof(A) == 344                      # the stream's extras travel beside the struct (include/smx.h)
    assert "smx_tbeam_resume" in _lib.SIGNATURES and "smx_tbeam_select_stream" in _lib.SIGNATURES
    lib = _lib.lib()
    resume, select = lib.smx_tbeam_resume, lib.smx_tbeam_select_stream
    assert lib.smx_tbeam_state_bytes(_lib.F32, 1, 64, 4, 16, 32, 0, 0) % 16 == 0
    # refused on the host, before any launch (the pointers are fake and never dereferenced)
    base = 1 << 40
    names = ("enc", "WihT", "bias", "Whh", "Wproj", "Wlin", "cur_tok", "h_in", "c_in", "h_out", "c_out", "pdec", "z", "state", "done", "overflow",
             "expansions", "frames", "tokens", "out_len", "scores", "sums", "n_hyps", "lengths")
    start, total = base + 4096 * 40, base + 4096 * 41

    def args(**kw):
        a = A(ld_b=64 * 8, ld_t=64, ldw=256, lm_weight=0.0, state_beam=2.3, expand_beam=2.3, dtype=_lib.F32, B=2, T=8, H=64, J=64, V=20, W=4,
              nbest=1, E=16, U=32, act=_lib.ACT_GELU, blank=0, **{n: base + 4096 * i for i, n in enumerate(names)})
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    EINVAL, EUNSUPPORTED = -1, -2
    entries = (lambda a, s=start, t=total: resume(ctypes.byref(a), s, t, None), lambda a, s=None, t=total: select(ctypes.byref(a), t, None))
    for entry in entries:
        assert entry(args(lengths=None)) == EINVAL
        assert entry(args(state=None)) == EINVAL
        assert entry(args(), t=None) == EINVAL
        for size in ("B", "T", "W", "E", "U", "nbest"):
            assert entry(args(**{size: 0})) == EINVAL, size
        assert entry(args(nbest=5)) == EINVAL
        assert entry(args(done=None)) == EINVAL
        assert entry(args(W=33, nbest=1)) == EUNSUPPORTED
        assert entry(args(H=48)) == EUNSUPPORTED
        assert entry(args(E=4096)) == EUNSUPPORTED
        assert entry(args(state=base + 8)) == EUNSUPPORTED
    assert resume(ctypes.byref(args()), None, total, None) == EINVAL
    assert resume(None, start, total, None) == EINVAL and select(None, total, None) == EINVAL
    assert select(ctypes.byref(args(lm_logits=base)), total, None) == EINVAL


def _modules(V=20, H=32, J=64, blank=3):
    from summarymixing_amd.nnet.embedding import Embedding
    from summarymixing_amd.nnet.linear import Linear
    from summarymixing_amd.nnet.RNN import LSTM
    from summarymixing_amd.nnet.transducer import Transducer_joint
    emb = Embedding(V, consider_as_one_hot=True, blank_id=blank)
    return (emb, LSTM(H, input_size=V - 1), Linear(J, input_size=H, bias=False), Transducer_joint(joint="sum", nonlinearity=torch.nn.GELU),
            Linear(V, input_size=J))


def _host_only_stream(B=2, C=4, J=64, device="cpu"):
    """A TransducerBeamStream with no device behind it: what decode_chunk validates on the host, it must refuse before it touches any buffer."""
    from summarymixing_amd.nnet.transducer import TransducerBeamStream
    s = object.__new__(TransducerBeamStream)
    s.B, s.chunk_frames, s._started, s._calls = B, C, [False] * B, 0
    s.state = types.SimpleNamespace(enc=torch.zeros((B, C, J), device=device))
    return s


def test_stream_refuses_on_the_host_by_message():
    from summarymixing_amd.nnet.transducer import TransducerBeamStream
    emb, dec, proj, tj, lin = _modules()
    with pytest.raises(ValueError, match="max_symbols is required"):
        TransducerBeamStream(emb, dec, proj, tj, lin, 2, 4, 4, None)
    s = _host_only_stream()
    enc = torch.zeros(2, 4, 64)
    with pytest.raises(ValueError, match="made for chunks"):
        s.decode_chunk(torch.zeros(2, 5, 64))
    with pytest.raises(ValueError, match="made for chunks"):
        s.decode_chunk(enc.bfloat16())
    with pytest.raises(ValueError, match="made for chunks"):
        _host_only_stream(device="meta").decode_chunk(enc)
    with pytest.raises(ValueError, match=r"outside \[0, chunk_frames = 4\]"):
        s.decode_chunk(enc, lengths=[4, 5])
    with pytest.raises(ValueError, match=r"outside \[0, chunk_frames = 4\]"):
        s.decode_chunk(enc, lengths=[-1, 0])
    with pytest.raises(ValueError, match="one entry per slot"):
        s.decode_chunk(enc, lengths=[4])
    with pytest.raises(ValueError, match=r"slots \[1\], which were never started"):
        s.decode_chunk(enc, lengths=[0, 2], start=[True, False])
    s._calls = 3                                         # start=None after the first call: nobody starts
    with pytest.raises(ValueError, match=r"slots \[0, 1\], which were never started"):
        s.decode_chunk(enc)
    assert s._started == [False, False] and s._calls == 3           # a refused call leaves the stream's bookkeeping alone


def test_forward_chunk_refuses_on_the_host_by_message():
    from summarymixing_amd.decoders.transducer_beam import TransducerBeamSearcher, TransducerStreamContext
    emb, dec, proj, tj, lin = _modules()
    beam = TransducerBeamSearcher([emb, dec, proj], tj, [lin], blank_id=3, beam_size=4, nbest=1)
    with pytest.raises(ValueError, match="max_symbols"):
        beam.make_stream(2, 4, None)
    with pytest.raises(ValueError, match="chunk_frames"):
        beam.make_stream(2, 0, 16)
    with pytest.raises(TypeError, match="make_stream"):
        beam.forward_chunk(torch.zeros(2, 4, 64), object())
    ctx = TransducerStreamContext(2, 4, torch.float32, _host_only_stream())
    with pytest.raises(ValueError, match="never started"):
        beam.forward_chunk(torch.zeros(2, 4, 64), ctx, lengths=[1, 1], start=[False, True])
    with pytest.raises(ValueError, match="made for chunks"):
        beam.forward_chunk(torch.zeros(2, 3, 64), ctx)
    greedy = TransducerBeamSearcher([emb, dec, proj], tj, [lin], blank_id=3, beam_size=1, nbest=1)
    ctx = greedy.make_stream(2, 4, 16)
    assert ctx.search is None and ctx.greedy is None
    with pytest.raises(ValueError, match="made for chunks"):
        greedy.forward_chunk(torch.zeros(2, 5, 64), ctx)
    with pytest.raises(ValueError, match=r"integers in \[0, chunk_frames = 4\]"):
        greedy.forward_chunk(torch.zeros(2, 4, 64), ctx, lengths=[5, 0])
    with pytest.raises(ValueError, match="never started"):
        greedy.forward_chunk(torch.zeros(2, 4, 64), ctx, lengths=[2, 2], start=[True, False])
    assert ctx.calls == 0 and ctx.started == [False, False]
