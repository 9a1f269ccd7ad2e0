"""CPU-side checks of the transducer beam search: the float64 restatement (tests/_tbeam_ref.py) against an independent
hypothesis-by-hypothesis loop over torch.nn.LSTMCell / torch.nn.LSTM, the admissibility of every case the GPU test decodes
token-exactly, the cap case, the new searcher's refusals and the C-ABI struct."""
import ctypes

import pytest
import torch

from tests import _greedy_ref as G
from tests import _tbeam_ref as R


# ---- the independent loop: torch.nn modules, hypotheses as tuples, sorting instead of arg-max picks
def _nn_modules(p, lm, blank):
    V, J = p["w_lin"].shape
    H = p["w_hh"].shape[1]
    cell = torch.nn.LSTMCell(V - 1, H).double()
    with torch.no_grad():
        cell.weight_ih.copy_(p["w_ih"]); cell.weight_hh.copy_(p["w_hh"]); cell.bias_ih.copy_(p["b_ih"]); cell.bias_hh.copy_(p["b_hh"])
    net = None
    if lm is not None:
        E = lm["embedding.Embedding.weight"].shape[1]
        Hl, D = lm["rnn.rnn.weight_hh_l0"].shape[1], lm["dnn.linear.w.weight"].shape[0]
        emb, rnn = torch.nn.Embedding(V, E).double(), torch.nn.LSTM(E, Hl, R.LM_LAYERS, batch_first=True).double()
        l1, ln, l2 = torch.nn.Linear(Hl, D).double(), torch.nn.LayerNorm(D).double(), torch.nn.Linear(D, V).double()
        with torch.no_grad():
            emb.weight.copy_(lm["embedding.Embedding.weight"])
            for k in range(R.LM_LAYERS):
                for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                    getattr(rnn, f"{n}_l{k}").copy_(lm[f"rnn.rnn.{n}_l{k}"])
            l1.weight.copy_(lm["dnn.linear.w.weight"]); l1.bias.copy_(lm["dnn.linear.w.bias"])
            ln.weight.copy_(lm["dnn.norm.norm.weight"]); ln.bias.copy_(lm["dnn.norm.norm.bias"])
            l2.weight.copy_(lm["out.w.weight"]); l2.bias.copy_(lm["out.w.bias"])
        net = (emb, rnn, torch.nn.Sequential(l1, ln, torch.nn.LeakyReLU(0.01), l2))
    return cell, net


@torch.no_grad()
def _independent(p, enc1, blank, W, lm):
    V = p["w_lin"].shape[0]
    H = p["w_hh"].shape[1]
    cell, net = _nn_modules(p, lm, blank)
    onehot = torch.eye(V, dtype=torch.float64)[:, [k for k in range(V) if k != blank]]       # the blank: a zero row
    closed = [((blank,), 0.0, None, None)]
    for t in range(enc1.shape[0]):
        opened, closed = list(closed), []
        while len(closed) < W:
            ranked = sorted(range(len(opened)), key=lambda i: (-opened[i][1] / len(opened[i][0]), i))
            pred, s, dec, lms = opened[ranked[0]]
            if closed:
                bs = sorted(closed, key=lambda h: -h[1] / len(h[0]))[0][1]
                if bs >= R.STATE_BEAM + s:
                    break
            del opened[ranked[0]]
            h2, c2 = cell(onehot[pred[-1]].view(1, -1), dec)
            out = h2 @ p["w_proj"].double().t()
            lp = torch.log_softmax(torch.nn.functional.linear(torch.nn.functional.gelu(enc1[t].double() + out), p["w_lin"].double(), p["b_lin"].double()), -1).view(-1)
            if net is not None:
                y, lm2 = net[1](net[0](torch.tensor([[pred[-1]]])), lms)
                lm_lp = torch.log_softmax(net[2](y).view(-1), -1)
            v, idx = torch.topk(lp, W)
            best = float(v[0]) if int(idx[0]) != blank else float(v[1])
            for vj, k in zip(v.tolist(), idx.tolist()):
                if k == blank:
                    closed.append((pred, s + vj, dec, lms))
                elif vj >= best - R.EXPAND_BEAM:
                    opened.append((pred + (k,), s + vj + (R.LM_WEIGHT * float(lm_lp[k]) if net is not None else 0.0), (h2, c2), lm2 if net is not None else None))
    closed = sorted(closed, key=lambda h: -h[1] / len(h[0]))
    return [(list(h[0][1:]), h[1]) for h in closed]


@pytest.mark.parametrize("name,use_lm", [("small", True), ("blank7", False)])
def test_restatement_equals_an_independent_loop(name, use_lm):
    p, enc, blank, W, lm, lengths = R.case(name, use_lm)
    ref = R.reference(name, use_lm)[0]
    got = _independent(p, enc[0], blank, W, lm)
    assert [h[0] for h in got] == [h[0] for h in ref["hyps"]]
    assert max(abs(g[1] - h[1]) for g, h in zip(got, ref["hyps"])) < 1e-9
    assert ref["overflow"] == 0


@pytest.mark.parametrize("name", tuple(R.CASES))
@pytest.mark.parametrize("use_lm", [False, True], ids=["nolm", "lm"])
def test_cases_are_admissible(name, use_lm):
    """On the reference alone, for every row of every case the GPU test decodes token-exactly."""
    p, enc, blank, W, lm, lengths = R.case(name, use_lm)
    assert enc.shape[0] == R.N_ROWS[name]
    exits, kinds, ties, pruned = set(), set(), [], 0
    for b in range(enc.shape[0]):
        if lengths[b] == 0:
            continue
        ref, emu = R.ref_and_emu(p, enc[b], blank, W, lm, n_frames=lengths[b])
        assert ref["hyps"] == R.reference(name, use_lm)[b]["hyps"]
        ok, mg, dev = R.admissible(ref, emu)
        print(f"{name} lm={use_lm} row {b}: smallest margin {mg:.2e}, largest deviation {dev:.2e}, {ref['expansions']} expansions")
        assert [h[0] for h in emu["hyps"]] == [h[0] for h in ref["hyps"]]
        assert mg >= 8 * dev and ref["overflow"] == 0 and emu["overflow"] == 0 and len(ref["hyps"][0][0]) > 0 and ok
        kinds |= {k for k, _ in ref["margins"]}
        ties += ref["ties"]
        assert emu["ties"] == ref["ties"]
        exits |= set(ref["exits"])
        pruned += ref["pruned"]
    assert {"count", "state"} <= exits and "cap" not in exits and "empty" not in exits
    assert pruned >= 1
    assert {"pick a", "pick b", "state_beam", "top-k", "expand_beam", "final sort"} <= kinds      # every kind of decision is taken and logged
    # exact ties (left out of the margin: list and index order settle them) occur in the tie case alone - there between the two tied
    # columns of the top-k in every row set and, without the LM, between the keys of their two children - and nowhere else
    if name == "tie":
        assert "top-k" in ties and (use_lm or "pick a" in ties) and set(ties) <= {"top-k", "pick a"}
    else:
        assert ties == []


def test_cap_case_sets_both_bits_and_stays_inside_the_caps():
    Bc, T, V, H, J, blank, W, seed, E, U = R.CAP
    p, enc = G.make_case(Bc, T, V, H, J, blank, seed)
    for b in range(Bc):
        free = R.search(p, enc[b], blank, W, None, E=10 ** 6, U=60)
        assert free["overflow"] & 2 or max(len(h[0]) for h in free["hyps"]) > U        # the model runs away when nothing holds it
        ref = R.search(p, enc[b], blank, W, None, E=E, U=U)
        assert ref["overflow"] == 3 and "cap" in ref["exits"]
        assert ref["expansions"] <= T * E and max(len(h[0]) for h in ref["hyps"]) <= U
        emu = R.ref_and_emu(p, enc[b], blank, W, None, E=E, U=U)[1]
        assert [h[0] for h in emu["hyps"]] == [h[0] for h in ref["hyps"]] and R.admissible(ref, emu)[1] >= 8 * R.deviation(ref, emu)


def _modules(V=20, H=32, J=64, blank=3):
    from summarymixing_amd.nnet.embedding import Embedding
    from summarymixing_amd.nnet.linear import Linear
    from summarymixing_amd.nnet.RNN import LSTM
    from summarymixing_amd.nnet.transducer import Transducer_joint
    emb = Embedding(V, consider_as_one_hot=True, blank_id=blank)
    return (emb, LSTM(H, input_size=V - 1), Linear(J, input_size=H, bias=False), Transducer_joint(joint="sum", nonlinearity=torch.nn.GELU),
            Linear(V, input_size=J))


def test_new_searcher_refuses_by_name_and_the_old_one_refuses_as_before():
    from summarymixing_amd.decoders.transducer import TransducerBeamSearcher as Old
    from summarymixing_amd.decoders.transducer_beam import TransducerBeamSearcher
    from summarymixing_amd.lobes.models.RNNLM import RNNLM
    emb, dec, proj, tj, lin = _modules()
    mods = torch.nn.ModuleDict(dict(emb=emb, dec=dec, proj_dec=proj, Tjoint=tj, transducer_lin=lin))
    keys = list(mods.state_dict().keys())
    lm = RNNLM(20, embedding_dim=32, rnn_layers=2, rnn_neurons=32, dnn_neurons=32, dropout=0.0, return_hidden=True)
    s = TransducerBeamSearcher([emb, dec, proj], tj, [lin], blank_id=3, beam_size=10, nbest=1, lm_module=lm, lm_weight=0.5, state_beam=2.3,
                               expand_beam=2.3)
    assert list(s.state_dict().keys()) == [] and list(s.parameters()) == []
    mods["searcher"] = s
    assert list(mods.state_dict().keys()) == keys
    with pytest.raises(NotImplementedError, match="nbest"):
        TransducerBeamSearcher([emb, dec, proj], tj, [lin], blank_id=3, beam_size=4, nbest=5)
    with pytest.raises(NotImplementedError, match="lm_module"):
        TransducerBeamSearcher([emb, dec, proj], tj, [lin], blank_id=3, beam_size=4, nbest=1, lm_module=torch.nn.Identity())
    with pytest.raises(NotImplementedError, match="return_hidden"):
        TransducerBeamSearcher([emb, dec, proj], tj, [lin], blank_id=3, beam_size=4, nbest=1,
                               lm_module=RNNLM(20, embedding_dim=32, rnn_neurons=32, dnn_neurons=32))
    with pytest.raises(NotImplementedError, match="decode_network_lst"):
        TransducerBeamSearcher([emb, dec], tj, [lin], blank_id=3, beam_size=4, nbest=1)
    with pytest.raises(NotImplementedError, match="beam_size"):
        TransducerBeamSearcher([emb, dec, proj], tj, [lin], blank_id=3, beam_size=64, nbest=1)
    with pytest.raises(ValueError):
        TransducerBeamSearcher([emb, dec, proj], tj, [lin], blank_id=0, beam_size=4, nbest=1)
    with pytest.raises(RuntimeError, match="GPU only"):
        s(torch.randn(1, 4, 64))
    with pytest.raises(NotImplementedError, match="beam search"):
        Old([emb, dec, proj], tj, [lin], blank_id=3, beam_size=4)
    with pytest.raises(NotImplementedError, match="beam search"):
        Old([emb, dec, proj], tj, [lin], blank_id=3, beam_size=1, lm_module=lm)


def test_abi_struct_and_host_side_refusals():
    from summarymixing_amd import _lib
    A = _lib.TbeamArgs
    assert ctypes.sizeof(A) == 344                      # see include/smx.h smx_tbeam_args
    assert A.enc.offset == 0 and A.lengths.offset == 24 and A.ldw.offset == 40 and A.blin.offset == 80 and A.cur_tok.offset == 88
    assert A.z.offset == 136 and A.lm_logits.offset == 144 and A.ld_lm.offset == 152 and A.state.offset == 192 and A.done.offset == 200
    assert A.n_hyps.offset == 264 and A.lm_weight.offset == 272 and A.dtype.offset == 284 and A.E.offset == 316 and A.U.offset == 320
    assert A.lm_H.offset == 336 and A.pad_.offset == 340
    lib = _lib.lib()
    ok = lib.smx_tbeam_ok
    assert ok(_lib.F32, 512, 640, 1000, 10) == 1 and ok(_lib.BF16, 512, 640, 1000, 10) == 1 and ok(_lib.BF16, 32, 64, 12, 3) == 1
    assert ok(_lib.F32, 48, 64, 20, 4) == 0 and ok(_lib.F32, 64, 96, 20, 4) == 0 and ok(_lib.F32, 64, 64, 20, 1) == 0
    assert ok(_lib.F32, 64, 64, 20, 33) == 0 and ok(_lib.F32, 64, 64, 4, 4) == 0 and ok(_lib.F32, 64, 64, 8193, 4) == 0 and ok(5, 64, 64, 20, 4) == 0
    small = lib.smx_tbeam_state_bytes(_lib.F32, 1, 64, 4, 16, 32, 0, 0)
    assert small > 0 and small % 16 == 0 and lib.smx_tbeam_state_bytes(_lib.F32, 3, 64, 4, 16, 32, 0, 0) == 3 * small
    assert lib.smx_tbeam_state_bytes(_lib.F32, 1, 64, 4, 16, 32, 2, 32) > small and lib.smx_tbeam_state_bytes(9, 1, 64, 4, 16, 32, 0, 0) == 0
    # refused on the host, before any launch (the pointers are fake and never dereferenced)
    base = 1 << 40
    def args(**kw):
        ptr = {n: base + 4096 * i for i, n in enumerate(("enc", "WihT", "bias", "Whh", "Wproj", "Wlin", "cur_tok", "h_in", "c_in", "h_out", "c_out",
                                                         "pdec", "z", "state", "done", "overflow", "expansions", "frames", "tokens", "out_len",
                                                         "scores", "sums", "n_hyps"))}
        a = A(ld_b=64 * 12, ld_t=64, ldw=256, lm_weight=0.0, state_beam=2.3, expand_beam=2.3, dtype=_lib.F32, B=2, T=12, H=64, J=64, V=20, W=4,
              nbest=1, E=16, U=32, act=_lib.ACT_GELU, blank=0, **ptr)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    EINVAL, EUNSUPPORTED = -1, -2
    for entry in (lib.smx_tbeam_init, lib.smx_tbeam_step, lib.smx_tbeam_select):
        assert entry(ctypes.byref(args(z=None)), None) == EINVAL
        assert entry(ctypes.byref(args(nbest=5)), None) == EINVAL
        assert entry(ctypes.byref(args(blank=20)), None) == EINVAL
        assert entry(ctypes.byref(args(h_out=base + 4096 * 7)), None) == EINVAL
        assert entry(ctypes.byref(args(lm_L=2)), None) == EINVAL
        assert entry(ctypes.byref(args(W=33, nbest=1)), None) == EUNSUPPORTED
        assert entry(ctypes.byref(args(H=48)), None) == EUNSUPPORTED
        assert entry(ctypes.byref(args(E=4096)), None) == EUNSUPPORTED
        assert entry(ctypes.byref(args(enc=base + 8)), None) == EUNSUPPORTED
    assert lib.smx_tbeam_select(ctypes.byref(args(lm_logits=base)), None) == EINVAL
