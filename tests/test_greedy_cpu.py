"""CPU checks of greedy transducer decoding: the float64 reference of tests/_greedy_ref.py against an independent loop, the
admissibility of the cases the GPU tests decode token-exactly, the start state, and the searcher's surface.  No GPU."""
import pytest
import torch

from tests import _greedy_ref as R


def _independent(p, enc, blank):
    """Row by row, frame by frame, with torch.nn.LSTMCell on explicit one-hot rows and torch.nn.functional: float64."""
    B, T, J = enc.shape
    V, H = p["w_lin"].shape[0], p["w_hh"].shape[1]
    cell = torch.nn.LSTMCell(V - 1, H).double()
    with torch.no_grad():
        cell.weight_ih.copy_(p["w_ih"]); cell.weight_hh.copy_(p["w_hh"]); cell.bias_ih.copy_(p["b_ih"]); cell.bias_hh.copy_(p["b_hh"])
    eye = torch.eye(V, dtype=torch.float64)
    table = torch.cat([eye[:, :blank], eye[:, blank + 1:]], 1)
    table[blank] = 0
    hyps, frames, scores = [], [], []
    with torch.no_grad():
        for b in range(B):
            h, c = cell(table[blank].view(1, -1))
            hyp, fr, sc = [], [], 0.0
            for t in range(T):
                a = torch.nn.functional.gelu(enc[b, t].double() + torch.nn.functional.linear(h, p["w_proj"].double()))
                lp = torch.log_softmax(torch.nn.functional.linear(a, p["w_lin"].double(), p["b_lin"].double()), -1).view(-1)
                k = int(lp.argmax())
                if k != blank:
                    hyp.append(k); fr.append(t); sc += float(lp[k])
                    h, c = cell(table[k].view(1, -1), (h, c))
            hyps.append(hyp); frames.append(fr); scores.append(sc)
    return hyps, frames, torch.tensor(scores, dtype=torch.float64)


@pytest.mark.parametrize("name", ["small", "blank7", "two_tiles", "v300"])
def test_reference_agrees_with_an_independent_loop(name):
    p, enc, blank = R.case(name)
    ref = R.decode(p, enc, blank)
    hyps, frames, scores = _independent(p, enc, blank)
    assert ref["hyps"] == hyps and ref["frames"] == frames
    assert float((ref["scores"] - scores).abs().max()) < 1e-9 * max(1.0, float(scores.abs().max()))


@pytest.mark.parametrize("name", R.EXACT + ("tie",))
def test_cases_are_admissible(name):
    """What the token-exact fp32 GPU test relies on, asserted on the reference alone: the fp32 emulation decodes the reference's exact
    sequence, the reference's smallest gap is >= 8 x the emulation's largest logit deviation, and both branches run."""
    p, enc, blank = R.case(name)
    exclude = R.TIE[8] if name == "tie" else None
    ref, emu = R.ref_and_emu(p, enc, blank, torch.float32, exclude=exclude)
    assert emu["hyps"] == ref["hyps"] and emu["frames"] == ref["frames"]
    dev = float((emu["z"].double() - ref["z"]).abs().max())
    gap = float(ref["gap"].min())
    assert gap >= 8 * dev, (gap, dev)
    B, T = enc.shape[:2]
    if B * T >= R.MIN_FRAMES_FOR_MIX:
        assert 0.25 <= float(ref["n"].sum()) / (B * T) <= 0.75
    if name == "tie":       # the lower twin wins at least twice, the upper never
        k1, k2 = R.TIE[7], R.TIE[8]
        assert sum(h.count(k1) for h in ref["hyps"]) >= 2 and sum(h.count(k2) for h in ref["hyps"]) == 0
        assert float((ref["z"][..., k1] - ref["z"][..., k2]).abs().max()) == 0.0


def test_lengths_and_chunks_in_the_reference():
    p, enc, blank = R.case("small")
    whole = R.decode(p, enc, blank)
    a = R.decode(p, enc[:, :7], blank)
    b = R.decode(p, enc[:, 7:], blank, state=a["state"])
    assert [x + y for x, y in zip(a["hyps"], b["hyps"])] == whole["hyps"]
    assert [x + y for x, y in zip(a["frames"], b["frames"])] == whole["frames"]
    assert torch.equal(b["scores"], whole["scores"]) and all(torch.equal(x, y) for x, y in zip(b["state"], whole["state"]))
    cut = R.decode(p, enc, blank, lengths=torch.tensor([24, 7, 0]))
    assert cut["hyps"][1] == a["hyps"][1] and cut["hyps"][2] == [] and cut["hyps"][0] == whole["hyps"][0]
    assert torch.equal(cut["state"][0][1], a["state"][0][1])


def test_start_state_is_the_blank_step_not_zeros():
    p, enc, blank = R.case("small")
    h, c, pdec = R.start_state(p, 2)
    b = (p["b_ih"] + p["b_hh"]).double()
    H = h.shape[1]
    cc = torch.sigmoid(b[:H]) * torch.tanh(b[2 * H:3 * H])
    assert torch.allclose(c[0], cc, atol=1e-12) and torch.allclose(h[0], torch.sigmoid(b[3 * H:]) * torch.tanh(cc), atol=1e-12)
    assert float(h.abs().max()) > 1e-3 and float(pdec.abs().max()) > 1e-3
    zero = (torch.zeros_like(h), torch.zeros_like(c), torch.zeros_like(pdec), torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.float64))
    assert not torch.equal(R.decode(p, enc[:2], blank)["z"], R.decode(p, enc[:2], blank, state=zero)["z"])


def _modules(V=20, H=32, J=64, blank=3, bias=True):
    from summarymixing_amd.nnet.embedding import Embedding
    from summarymixing_amd.nnet.linear import Linear
    from summarymixing_amd.nnet.RNN import LSTM
    from summarymixing_amd.nnet.transducer import Transducer_joint
    emb = Embedding(V, consider_as_one_hot=True, blank_id=blank)
    return (emb, LSTM(H, input_size=V - 1), Linear(J, input_size=H, bias=False), Transducer_joint(joint="sum", nonlinearity=torch.nn.GELU),
            Linear(V, input_size=J, bias=bias))


def test_searcher_refuses_beam_search_and_an_lm_and_adds_no_state():
    from summarymixing_amd.decoders.transducer import TransducerBeamSearcher
    emb, dec, proj, tj, lin = _modules()
    mods = torch.nn.ModuleDict(dict(emb=emb, dec=dec, proj_dec=proj, Tjoint=tj, transducer_lin=lin))
    keys = list(mods.state_dict().keys())
    s = TransducerBeamSearcher([emb, dec, proj], tj, [lin], blank_id=3, beam_size=1, nbest=1, lm_module=None, lm_weight=0.0,
                               state_beam=2.3, expand_beam=2.3)
    assert list(s.state_dict().keys()) == [] and list(s.parameters()) == [] and list(mods.state_dict().keys()) == keys
    mods["searcher"] = s
    assert list(mods.state_dict().keys()) == keys
    with pytest.raises(NotImplementedError, match="beam search"):
        TransducerBeamSearcher([emb, dec, proj], tj, [lin], blank_id=3, beam_size=4)
    with pytest.raises(NotImplementedError, match="beam search"):
        TransducerBeamSearcher([emb, dec, proj], tj, [lin], blank_id=3, beam_size=1, lm_module=torch.nn.Identity())
    with pytest.raises(ValueError):
        TransducerBeamSearcher([emb, dec, proj], tj, [lin], blank_id=0, beam_size=1)


def test_no_cpu_fallback_and_unsupported_shapes_raise_before_any_launch():
    from summarymixing_amd.nnet.transducer import greedy_decode
    emb, dec, proj, tj, lin = _modules()
    with pytest.raises(RuntimeError, match="GPU only"):
        greedy_decode(torch.randn(1, 4, 64), emb, dec, proj, tj, lin)
    from summarymixing_amd import _lib
    ok = _lib.lib().smx_greedy_ok
    assert ok(_lib.F32, 512, 640, 1000) == 1 and ok(_lib.BF16, 32, 64, 2) == 1
    assert ok(_lib.F32, 48, 64, 20) == 0 and ok(_lib.F32, 64, 96, 20) == 0 and ok(_lib.F32, 64, 64, 1) == 0 and ok(5, 64, 64, 20) == 0
    assert _lib.lib().smx_greedy_workspace(17, 300) >= 17 * 3 * 12
    # refused on the host, before any launch (the pointers are fake and never dereferenced)
    base = 1 << 40
    rc = _lib.lib().smx_greedy_start(_lib.F32, base, base, base, base, base, base, 2, 64, 96, None)
    assert rc == -2
