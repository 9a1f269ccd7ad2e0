"""Transducer beam search on the GPU (csrc/tbeam.hip behind nnet.transducer.beam_decode, CapturedTransducerBeam and
decoders.transducer_beam.TransducerBeamSearcher) against the float64 restatement tests/_tbeam_ref.py on the same parameters and inputs.

float32 decodes the reference's exact hypotheses, in its order, on cases the CPU suite proves admissible (test_tbeam_cpu.py: the
smallest margin of every decision >= 8 x the fp32 emulation's largest deviation).  A free-running bf16 search cannot be asked that, so
both dtypes are also judged (a) per expansion, on the reference's own trajectory, within bar = max(TOL, 4 x floor), the floor being the
emulation's deviation on that trajectory, and (b) against a host loop of Python lists over the same arithmetic entry.  Everything else
is bit equality."""
import pytest
import torch

from tests import _greedy_ref as G
from tests import _tbeam_ref as R
from tests._util import TOL, rel_err, report

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
NAMES = tuple(R.CASES)
BOTH = [(n, lm) for n in NAMES for lm in (False, True)]
IDS = [f"{n}-{'lm' if lm else 'nolm'}" for n, lm in BOTH]


def _mods(p, blank):
    from summarymixing_amd.nnet.embedding import Embedding
    from summarymixing_amd.nnet.linear import Linear
    from summarymixing_amd.nnet.RNN import LSTM
    from summarymixing_amd.nnet.transducer import Transducer_joint
    V, J = p["w_lin"].shape
    H = p["w_hh"].shape[1]
    emb, dec, proj = Embedding(V, consider_as_one_hot=True, blank_id=blank), LSTM(H, input_size=V - 1), Linear(J, input_size=H, bias=False)
    tj, lin = Transducer_joint(joint="sum", nonlinearity=torch.nn.GELU), Linear(V, input_size=J)
    with torch.no_grad():
        dec.rnn.weight_ih_l0.copy_(p["w_ih"]); dec.rnn.weight_hh_l0.copy_(p["w_hh"])
        dec.rnn.bias_ih_l0.copy_(p["b_ih"]); dec.rnn.bias_hh_l0.copy_(p["b_hh"])
        proj.w.weight.copy_(p["w_proj"]); lin.w.weight.copy_(p["w_lin"]); lin.w.bias.copy_(p["b_lin"])
    return tuple(m.cuda() for m in (emb, dec, proj, tj, lin))


def _lm_module(sd, dtype):
    from summarymixing_amd.lobes.models.RNNLM import RNNLM
    V, E = sd["embedding.Embedding.weight"].shape
    H, D = sd["rnn.rnn.weight_hh_l0"].shape[1], sd["dnn.linear.w.weight"].shape[0]
    lm = RNNLM(V, embedding_dim=E, rnn_layers=R.LM_LAYERS, rnn_neurons=H, dnn_neurons=D, dropout=0.0, return_hidden=True)
    lm.load_state_dict(sd, strict=True)
    lm = lm.cuda().eval()
    return lm.bfloat16() if dtype == BF16 else lm


_cache = {}


def _setup(name, use_lm, dtype=F32):
    """(modules, LM module or None, enc on the GPU, lengths on the GPU, W, the CPU case) of a named case, built once."""
    key = (name, use_lm, dtype)
    if key not in _cache:
        c = R.case(name, use_lm, dtype)
        p, enc, blank, W, lm, lengths = c
        _cache[key] = (_mods(p, blank), _lm_module(lm, dtype) if use_lm else None, enc.cuda().to(dtype),
                       torch.tensor(lengths, dtype=torch.int32).cuda(), W, c)
    return _cache[key]


def _decode(name, use_lm, dtype=F32, nbest=None, rows=None, **kw):
    from summarymixing_amd.nnet.transducer import beam_decode
    mods, lm, enc, lengths, W, _ = _setup(name, use_lm, dtype)
    if rows is not None:
        enc, lengths = enc[rows], lengths[rows]
    return beam_decode(enc, *mods, W, nbest=W if nbest is None else nbest, lm=lm, lm_weight=R.LM_WEIGHT, state_beam=R.STATE_BEAM,
                       expand_beam=R.EXPAND_BEAM, lengths=lengths, **kw)


def _host(r):
    return type(r)(*(t.cpu() for t in r))


def _hyps(r, b):
    """[(tokens, sum, key)] of utterance b of a host result; checks the padding."""
    out = []
    for i in range(int(r.n_hyps[b])):
        n = int(r.lengths[b, i])
        assert bool((r.tokens[b, i, :n] >= 0).all()) and bool((r.tokens[b, i, n:] == -1).all()), "tokens are not padded with -1 after lengths"
        out.append((r.tokens[b, i, :n].tolist(), float(r.sums[b, i]), float(r.scores[b, i])))
    assert bool((r.lengths[b, int(r.n_hyps[b]):] == 0).all()) and bool((r.tokens[b, int(r.n_hyps[b]):] == -1).all())
    return out


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _assert_equals_search(r, b, ref, nbest, what):
    got = _hyps(r, b)
    want = ref["hyps"][:nbest]
    assert [h[0] for h in got] == [h[0] for h in want], f"{what} row {b}: hypotheses differ from the reference's"
    scale = max(1.0, max(abs(h[1]) for h in want))
    es = max((abs(g[1] - w[1]) for g, w in zip(got, want)), default=0.0) / scale
    ek = max((abs(g[2] - w[2]) for g, w in zip(got, want)), default=0.0) / scale
    print(f"{what} row {b}: sum err {es:.2e} key err {ek:.2e} (bar {TOL[F32][0]:.0e})")
    assert es <= TOL[F32][0] and ek <= TOL[F32][0]
    assert int(r.expansions[b]) == ref["expansions"] and int(r.frames[b]) == ref["frames"] and int(r.overflow[b]) == ref["overflow"]
    return es, ek


# ---- 1. the arithmetic entry against fp64, per expansion, on the reference's own trajectory
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", NAMES)
def test_arithmetic_entry_on_the_reference_trajectory(name, dtype):
    from summarymixing_amd import ops
    from summarymixing_amd.nnet.transducer import beam as Bm
    mods, _, enc, lengths, W, (p, enc_cpu, blank, _, _, lens) = _setup(name, False, dtype)
    rnd = G.rounder(dtype)
    traj = []
    for b in range(enc_cpu.shape[0]):
        ref = R.search(p, enc_cpu[b], blank, W, None, n_frames=lens[b])
        traj += [(b, e) for e in ref["traj"]]
    traj = traj[:64]
    n = len(traj)
    encs = torch.stack([enc_cpu[b] for b, _ in traj]).cuda().to(dtype)
    st = Bm._make_state(encs, *mods, W, 1, None, 0.0, R.STATE_BEAM, R.EXPAND_BEAM, None, None)
    st.begin(encs, None)
    st.cur_tok.copy_(torch.tensor([e["tok"] for _, e in traj], dtype=torch.int32))
    st.frames.copy_(torch.tensor([e["t"] for _, e in traj], dtype=torch.int32))
    h_in = torch.cat([rnd(e["h"].float()) for _, e in traj])
    c_in = torch.cat([e["c"].float() for _, e in traj])
    st.h_in.copy_(h_in.to(dtype)); st.c_in.copy_(c_in)
    ops.tbeam_step(st)
    # the reference and the emulation of ONE step from the inputs the device got
    toks = torch.tensor([e["tok"] for _, e in traj])
    worst = {}
    for which, dt, r in (("ref", torch.float64, lambda t: t), ("emu", torch.float32, rnd)):
        h2, c2 = G._lstm_step(p, toks, h_in.to(dt), c_in.to(dt), blank, dt)
        h2 = r(h2)
        pdec = r(h2 @ p["w_proj"].to(dt).t())
        e_t = torch.stack([enc_cpu[b][e["t"]] for b, e in traj]).to(dt)
        z = r(G.gelu(e_t + pdec)) @ p["w_lin"].to(dt).t() + p["b_lin"].to(dt)
        worst[which] = dict(h=h2, c=c2, pdec=pdec, z=z)
    entries = {}
    for k, got in (("h", st.h_out), ("c", st.c_out), ("pdec", st.pdec), ("z", st.z)):
        err, floor = rel_err(got, worst["ref"][k]), rel_err(worst["emu"][k], worst["ref"][k])
        bar = max(TOL[dtype][0], 4 * floor)
        entries[k] = dict(err=err, floor=floor, bar=bar)
        print(f"{name} {dtype} {k}: err {err:.2e} floor {floor:.2e} bar {bar:.2e}")
        assert err <= bar, (name, k, err, bar)
    report("tbeam_step", dict(case=name, dtype=str(dtype), rows=n, **entries))


# ---- 2. float32, free-running: the float64 search's hypotheses, order, counts
@pytest.mark.parametrize("name,use_lm", BOTH, ids=IDS)
def test_fp32_search_equals_the_float64_search(name, use_lm):
    W = R.CASES[name][5]
    r = _host(_decode(name, use_lm))
    refs = R.reference(name, use_lm)
    entries = []
    for b, ref in enumerate(refs):
        assert int(r.n_hyps[b]) == min(len(ref["hyps"]), W)
        es, ek = _assert_equals_search(r, b, ref, W, f"{name} lm={use_lm}")
        entries.append(dict(row=b, sum_err=es, key_err=ek, expansions=ref["expansions"]))
    report("tbeam_search", dict(case=name, lm=use_lm, rows=entries))
    if name == "small":
        assert int(r.n_hyps[1]) == 1 and int(r.lengths[1, 0]) == 0 and float(r.scores[1, 0]) == 0.0 and int(r.frames[1]) == 0


# ---- 3. both dtypes: the device search equals a host loop of Python lists over the same arithmetic entry and RNNLM.step
@torch.no_grad()
def _host_loop(name, use_lm, dtype, b):
    """The list logic of the restatement driving smx_tbeam_step and RNNLM.step one hypothesis at a time (B = 1); the log-softmax is
    torch's, in fp32.  -> [(tokens, sum)] sorted as the restatement sorts."""
    from summarymixing_amd import ops
    from summarymixing_amd.nnet.transducer import beam as Bm
    mods, lm, enc, lengths, W, (p, _, blank, _, _, lens) = _setup(name, use_lm, dtype)
    e1 = enc[b:b + 1]
    st = Bm._make_state(e1, *mods, W, 1, lm, R.LM_WEIGHT, R.STATE_BEAM, R.EXPAND_BEAM, None, None)
    st.begin(e1, None)
    H = st.H
    key = lambda h: h["s"] / torch.tensor(float(len(h["pred"])))
    best = lambda hs: int(torch.argmax(torch.stack([key(h) for h in hs])))
    zero = (torch.zeros(1, H, device="cuda", dtype=dtype), torch.zeros(1, H, device="cuda"))
    lm0 = None if lm is None else (torch.zeros_like(st.lm_h_in), torch.zeros_like(st.lm_c_in))
    Bh = [dict(pred=[blank], s=torch.zeros(()), dec=zero, lm=lm0)]
    for t in range(lens[b]):
        A, Bh, nexp = Bh, [], 0
        while len(Bh) < W and nexp < st.E and A:
            ia = best(A)
            a = A[ia]
            if Bh:
                bb = Bh[best(Bh)]
                if bb["s"] >= torch.tensor(R.STATE_BEAM) + a["s"]:
                    break
            A.pop(ia)
            nexp += 1
            st.cur_tok.fill_(a["pred"][-1]); st.frames.fill_(t)
            st.h_in.copy_(a["dec"][0]); st.c_in.copy_(a["dec"][1])
            ops.tbeam_step(st)
            lp = torch.log_softmax(st.z[0], -1).cpu()
            new = (st.h_out.clone(), st.c_out.clone())
            if lm is not None:
                logits, hid = lm.step(st.cur_tok, hx=a["lm"])
                lm_lp = torch.log_softmax(logits[0].float(), -1).cpu()
            v, idx = torch.sort(lp, descending=True, stable=True)
            top = v[0] if int(idx[0]) != blank else v[1]
            for j in range(W):
                k = int(idx[j])
                if k == blank:
                    Bh.append(dict(pred=a["pred"], s=a["s"] + v[j], dec=a["dec"], lm=a["lm"]))
                elif v[j] >= top - torch.tensor(R.EXPAND_BEAM):
                    s = a["s"] + v[j]
                    if lm is not None:
                        s = s + torch.tensor(R.LM_WEIGHT) * lm_lp[k]
                    A.append(dict(pred=a["pred"] + [k], s=s, dec=new, lm=hid if lm is not None else None))
    out, rest = [], list(Bh)
    while rest:
        out.append(rest.pop(best(rest)))
    return [(h["pred"][1:], float(h["s"])) for h in out]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name,use_lm", [("small", False), ("small", True), ("blank7", True), ("v300", False), ("tie", False), ("tie", True)],
                         ids=["small", "small-lm", "blank7-lm", "v300", "tie", "tie-lm"])
def test_device_search_equals_the_host_logic_loop(name, use_lm, dtype):
    """Same arithmetic, so the hypotheses must be equal; the sums differ by the log-softmax's last bits only.  The bound: torch's fp32
    log-softmax and the kernel's row code (fp32 exponentials, fp64 combination) each carry a relative error of a few 2^-24 on lse, i.e.
    an absolute error below 2^-20 on a log-probability of magnitude < 16; a hypothesis sums at most len + frames of them (the LM's
    share weighs 0.5), so |difference| <= 2^-19 x (symbols + frames + 1) x 2.  The tie case holds two bit-equal logit columns: the loop
    orders them with a stable sort and takes the first maximum among equal keys, so a selection that breaks ties to the higher index or
    the later insertion returns other hypotheses here."""
    W = R.CASES[name][5]
    r = _host(_decode(name, use_lm, dtype))
    lens = _setup(name, use_lm, dtype)[5][5]
    for b in (0, 2) if name == "small" else (0, 1):
        want = _host_loop(name, use_lm, dtype, b)
        got = _hyps(r, b)
        assert [h[0] for h in got] == [h[0] for h in want[:W]], (name, b)
        for g, w in zip(got, want):
            bound = 2.0 ** -19 * (len(g[0]) + lens[b] + 1) * 2
            assert abs(g[1] - w[1]) <= bound, (name, b, g[1], w[1], bound)


# ---- 4. the cap case
def test_cap_case_equals_the_restatement_and_sets_the_overflow_bits():
    from summarymixing_amd.nnet.transducer import beam_decode
    Bc, T, V, H, J, blank, W, seed, E, U = R.CAP
    p, enc = G.make_case(Bc, T, V, H, J, blank, seed)
    mods = _mods(p, blank)
    r = _host(beam_decode(enc.cuda(), *mods, W, nbest=W, max_expansions=E, max_symbols=U))
    for b in range(Bc):
        ref = R.search(p, enc[b], blank, W, None, E=E, U=U)
        assert ref["overflow"] == 3
        _assert_equals_search(r, b, ref, W, "cap")
        assert int(r.expansions[b]) <= T * E and int(r.lengths[b].max()) <= U


# ---- 5. independence and reproducibility
@pytest.mark.parametrize("use_lm", [False, True], ids=["nolm", "lm"])
def test_rows_do_not_depend_on_the_batch_and_runs_are_bit_equal(use_lm):
    whole = _decode("small", use_lm)
    again = _decode("small", use_lm)
    assert _same(whole, again)
    assert _same(whole, _decode("small", use_lm, poll_every=1))
    for b in range(3):
        one = _decode("small", use_lm, rows=[b])
        assert all(torch.equal(x[b:b + 1], y) for x, y in zip(whole, one)), f"row {b} of B = 3 differs from B = 1"


@pytest.mark.parametrize("use_lm", [False, True], ids=["nolm", "lm"])
def test_captured_equals_eager_on_two_inputs(use_lm):
    from summarymixing_amd.nnet.transducer import CapturedTransducerBeam
    mods, lm, enc, lengths, W, _ = _setup("small", use_lm)
    cap = CapturedTransducerBeam(*mods, enc.shape[0], enc.shape[1], W, nbest=W, lm=lm, lm_weight=R.LM_WEIGHT)
    eager = _decode("small", use_lm)
    got = cap.decode(enc, lengths)
    assert _same(eager, got)
    enc2 = enc.flip(0).contiguous()
    from summarymixing_amd.nnet.transducer import beam_decode
    eager2 = beam_decode(enc2, *mods, W, nbest=W, lm=lm, lm_weight=R.LM_WEIGHT)
    assert _same(eager2, cap.decode(enc2))
    assert not torch.equal(eager2.tokens, eager.tokens)


# ---- 6. the kernels write inside their outputs only
@torch.no_grad()
def test_outputs_live_inside_poisoned_buffers():
    from summarymixing_amd import ops
    from summarymixing_amd.nnet.transducer import beam as Bm
    mods, lm, enc, lengths, W, _ = _setup("b17", True)
    st = Bm._make_state(enc, *mods, W, W, lm, R.LM_WEIGHT, R.STATE_BEAM, R.EXPAND_BEAM, None, None)
    G_ = 64
    guarded = {}
    for name in ("h_in", "c_in", "h_out", "c_out", "pdec", "z", "cur_tok", "lm_h_in", "lm_c_in", "state", "done", "overflow", "expansions", "frames",
                 "tokens", "out_len", "scores", "sums", "n_hyps"):
        t = getattr(st, name)
        big = torch.empty(t.numel() + 2 * G_, dtype=t.dtype, device=t.device)
        big.view(torch.uint8).fill_(0xA5)
        inner = big[G_:G_ + t.numel()].view(t.shape)
        inner.copy_(t)
        setattr(st, name, inner)
        guarded[name] = (big, t.numel())
    st.begin(enc, lengths)
    Bm._poll_loop(st.step, st, 32)
    plain = _decode("b17", True)
    assert _same(plain, st.result())
    for name, (big, n) in guarded.items():
        raw = big.view(torch.uint8)
        es = big.element_size()
        assert bool((raw[:G_ * es] == 0xA5).all()) and bool((raw[(G_ + n) * es:] == 0xA5).all()), f"{name}: a guard was written"


# ---- 7. the module surface
def _searcher(name, use_lm, **kw):
    from summarymixing_amd.decoders.transducer_beam import TransducerBeamSearcher
    mods, lm, enc, lengths, W, (p, _, blank, _, _, _) = _setup(name, use_lm)
    emb, dec, proj, tj, lin = mods
    args = dict(beam_size=W, nbest=1, lm_module=lm, lm_weight=R.LM_WEIGHT if use_lm else 0.0, state_beam=R.STATE_BEAM, expand_beam=R.EXPAND_BEAM)
    args.update(kw)
    return TransducerBeamSearcher([emb, dec, proj], tj, [lin], blank, **args), enc


def test_module_returns_the_upstream_tuple():
    import math
    s, enc = _searcher("blank7", True)
    hyps, score, nbest_hyps, nbest_keys = s(enc)
    refs = R.reference("blank7", True)
    assert hyps == [r["hyps"][0][0] for r in refs]
    assert nbest_hyps == [[r["hyps"][0][0]] for r in refs] and [len(k) for k in nbest_keys] == [1, 1]
    want = sum(math.exp(r["hyps"][0][2]) for r in refs) / len(refs)
    assert abs(score - want) <= TOL[F32][0] * want
    assert list(s.state_dict().keys()) == [] and list(s.parameters()) == []


def test_module_nbest_three_best_first():
    s, enc = _searcher("blank7", False, nbest=3)
    hyps, score, nbest_hyps, nbest_keys = s(enc)
    refs = R.reference("blank7", False)
    for b, r in enumerate(refs):
        assert nbest_hyps[b] == [h[0] for h in r["hyps"][:3]] and len(nbest_hyps[b]) == 3
        assert nbest_keys[b] == sorted(nbest_keys[b], reverse=True) and hyps[b] == nbest_hyps[b][0]


def test_module_lm_weight_zero_equals_no_lm_bit_for_bit():
    from summarymixing_amd.nnet.transducer import beam_decode
    mods, lm, enc, lengths, W, _ = _setup("blank7", True)
    assert _same(beam_decode(enc, *mods, W, nbest=W, lm=lm, lm_weight=0.0), beam_decode(enc, *mods, W, nbest=W))
    with_lm, _ = _searcher("blank7", True, nbest=3, lm_weight=0.0)
    without, _ = _searcher("blank7", True, nbest=3, lm_module=None, lm_weight=0.0)
    assert with_lm.lm is lm and without.lm is None
    assert with_lm(enc) == without(enc)                      # (lists and floats from the one host copy: equal means bit-equal keys)


def test_module_reports_the_caps():
    """On a search that hits the caps the 4-tuple alone is silent: the module warns and keeps the per-utterance bits."""
    from summarymixing_amd.decoders.transducer_beam import TransducerBeamSearcher
    Bc, T, V, H, J, blank, W, seed, E, U = R.CAP
    p, enc = G.make_case(Bc, T, V, H, J, blank, seed)
    emb, dec, proj, tj, lin = _mods(p, blank)
    s = TransducerBeamSearcher([emb, dec, proj], tj, [lin], blank, beam_size=W, nbest=1, max_expansions=E, max_symbols=U)
    with pytest.warns(RuntimeWarning, match="max_expansions"):
        hyps, _, _, _ = s(enc.cuda())
    assert s.last_overflow == [3, 3] and hyps == [R.search(p, enc[b], blank, W, None, E=E, U=U)["hyps"][0][0] for b in range(Bc)]
    free, enc2 = _searcher("blank7", False)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        free(enc2)
    assert free.last_overflow == [0, 0]


def test_module_beam_one_equals_the_greedy_searcher():
    from summarymixing_amd.decoders.transducer import TransducerBeamSearcher as Greedy
    s, enc = _searcher("blank7", False, beam_size=1, nbest=1)
    emb, dec, proj = s.decode_network_lst
    g = Greedy([emb, dec, proj], s.tjoint, s.classifier_network, s.blank_id, beam_size=1, nbest=1)
    assert s(enc) == g(enc)
