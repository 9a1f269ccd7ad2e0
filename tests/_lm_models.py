"""The small language models of the TransformerLM tests (tests/test_transformerlm_*.py, tests/test_s2s_lm_beam_gpu.py), built like the
models of tests/_s2s_models.py - random non-trivial biases and LayerNorm parameters, everything rounded to the dtype - over the same
vocabulary, and their float64 / ATen restatements through tests/_transformerlm_ref.py."""
import torch
from torch import nn

from tests import _transformerlm_ref as LR
from tests._s2s_models import V, randomise

# name -> (d, H, d_ffn, layers, normalize_before); the last has the recipe's head count and head dimension (12 x 64)
MODELS = {"lm-d64-post": (64, 1, 128, 2, False), "lm-d128-h2-pre": (128, 2, 128, 2, True), "lm-d768-h12-post": (768, 12, 256, 1, False)}
MAX_LENGTH = 100


def build(name, dtype, seed, device="cuda"):
    """-> TransformerLM in eval mode on `device`, every parameter rounded to dtype."""
    from summarymixing_amd.lobes.models.transformer.TransformerLM import TransformerLM
    d, H, f, layers, pre = MODELS[name]
    torch.manual_seed(seed)
    m = TransformerLM(V, d_model=d, nhead=H, num_encoder_layers=layers, num_decoder_layers=0, d_ffn=f, dropout=0.0, activation=nn.GELU,
                      normalize_before=pre, max_length=MAX_LENGTH)
    randomise(m, dtype, seed + 1)
    return m.to(device).eval()


def restated(name, m, impl, dtype, device="cuda"):
    """fn(tokens (B, U) on the CPU, mask_pad=True) -> logits (B, U, V) of the whole sequences under the look-ahead mask: float64 on the
    CPU (impl="f64") or the ATen chain at `dtype` on `device` (impl="aten": the table and the embedding sum stay float32)."""
    d, H, f, layers, pre = MODELS[name]
    dev = "cpu" if impl == "f64" else device
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    P = {k: v.to(device=dev, dtype=torch.float64 if impl == "f64" else (torch.float32 if k in (LR.TABLE, LR.PE) else dtype)) for k, v in sd.items()}

    def fn(tokens, mask_pad=True):
        with torch.no_grad():
            return LR.lm(tokens.to(dev), P, layers, H, "gelu", pre, impl=impl, mask_pad=mask_pad,
                         dtype=torch.float64 if impl == "f64" else dtype)
    return fn
