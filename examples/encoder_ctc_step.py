#!/usr/bin/env python3
"""One multitask-CTC training step of the encoder side of the LibriSpeech Conformer-SummaryMixing recipe on the HIP path:
waveform -> Fbank -> InputNormalization -> ConvolutionFrontEnd -> TransformerASR.encode -> proj_enc -> proj_ctc ->
log_softmax -> ctc_cost, optimised by the flat-buffer AdamW (needs an MI355X; synthetic data).

    python examples/encoder_ctc_step.py [--steps 20] [--batch 16] [--seconds 8] [--augment] [--wav-augment] [--decode]
                                        [--noam-warmup N] [--sgd-after K]

--augment inserts the recipe's fea_augment (time drops, frequency drops, time warp: yaml:195-245) between the filterbank and the
normalisation, where upstream's transducer train.py applies it; off by default.
--wav-augment applies the recipe's wav_augment (SpeedPerturb at speeds 95 / 100 / 105: yaml:177-192) to the waveform batch before
the filterbank, where upstream's train.py applies it; off by default.
--decode prints, after the last step, the batch's hypotheses under CTC greedy decoding (speechbrain.decoders.ctc.ctc_greedy_decode:
row arg-max, merge repeats, drop the blank - on the device, one copy to the host at the end).
--noam-warmup N attaches the transformer recipes' NoamScheduler (lr_initial = the optimizer's rate, n_warmup_steps = N) to the
optimizer: the rate of every update is computed on the device (opt.lr_dev); the recipe's `noam_annealing(optimizer)` line stays.
--sgd-after K is the two-stage recipes' switch (AISHELL-1, CommonVoice: stage_one_epochs of Adam, then SGD with momentum 0.99 and
Nesterov): after K steps FlatSGD.adopt takes the flat buffers and shadows over in place and training goes on at a constant rate.

The module names and constructor arguments are the ones the reference YAML passes (…/LibriSpeech/ASR/transducer/
hparams/conformer_summarymixing_transducer.yaml); only the import root changes: speechbrain.* -> summarymixing_amd.*."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from summarymixing_amd.augment.augmenter import Augmenter                                     # noqa: E402
from summarymixing_amd.augment.freq_domain import SpectrogramDrop, Warping                  # noqa: E402
from summarymixing_amd.augment.time_domain import SpeedPerturb                               # noqa: E402
from summarymixing_amd.decoders import ctc_greedy_decode                                     # noqa: E402
from summarymixing_amd.lobes.features import Fbank, InputNormalization                     # noqa: E402
from summarymixing_amd.lobes.models.convolution import ConvolutionFrontEnd                   # noqa: E402
from summarymixing_amd.lobes.models.transformer.TransformerASR import EncoderWrapper, TransformerASR  # noqa: E402
from summarymixing_amd.nnet.activations import Softmax                                       # noqa: E402
from summarymixing_amd.nnet.linear import Linear                                             # noqa: E402
from summarymixing_amd.nnet.losses import ctc_loss                                           # noqa: E402
from summarymixing_amd.nnet.schedulers import NoamScheduler                                  # noqa: E402
from summarymixing_amd.trainer import FlatAdamW, FlatSGD                                     # noqa: E402


class EncoderSide(torch.nn.Module):
    def __init__(self, d_model=256, d_ffn=1024, layers=12, joint_dim=640, vocab=1000, augment=False, wav_augment=False):
        super().__init__()
        self.wav_augment = None
        if wav_augment:
            speed_perturb = SpeedPerturb(orig_freq=16000, speeds=[95, 100, 105])
            self.wav_augment = Augmenter(parallel_augment=False, concat_original=False, repeat_augment=1, shuffle_augmentations=False,
                                         min_augmentations=1, max_augmentations=1, augment_prob=1.0, augmentations=[speed_perturb])
        self.fea_augment = None
        if augment:
            time_drop = SpectrogramDrop(drop_length_low=15, drop_length_high=25, drop_count_low=5, drop_count_high=5,
                                        replace="zeros", dim=1)
            freq_drop = SpectrogramDrop(drop_length_low=25, drop_length_high=35, drop_count_low=2, drop_count_high=2,
                                        replace="zeros", dim=2)
            time_warp = Warping(warp_window=5, warp_mode="bicubic", dim=1)
            self.fea_augment = Augmenter(parallel_augment=False, concat_original=False, repeat_augment=1, shuffle_augmentations=False,
                                         min_augmentations=3, max_augmentations=3, augment_prob=1.0,
                                         augmentations=[time_drop, freq_drop, time_warp])
        self.compute_features = Fbank(sample_rate=16000, n_fft=512, n_mels=80, win_length=32)
        self.normalize = InputNormalization(norm_type="global", update_until_epoch=4)
        self.CNN = ConvolutionFrontEnd((None, None, 80), num_blocks=2, num_layers_per_block=1, out_channels=(64, 32),
                                       kernel_sizes=(3, 3), strides=(2, 2), residuals=(False, False))
        self.enc = EncoderWrapper(TransformerASR(
            tgt_vocab=vocab, input_size=640, d_model=d_model, nhead=4, num_encoder_layers=layers, num_decoder_layers=0,
            d_ffn=d_ffn, dropout=0.1, encoder_module="conformer", attention_type="SummaryMixing", mode="SummaryMixing-fast",
            local_proj_hid_dim=[d_model], local_proj_out_dim=d_model, summary_hid_dim=[d_model], summary_out_dim=d_model,
            causal=False))
        self.proj_enc = Linear(joint_dim, input_size=d_model)
        self.proj_ctc = Linear(vocab, input_size=joint_dim)
        self.log_softmax = Softmax(apply_log=True)

    def forward(self, wav, wav_lens, epoch=0):
        if self.wav_augment is not None and self.training:
            wav, wav_lens = self.wav_augment(wav, wav_lens)
        feats = self.compute_features(wav, out_dtype=torch.bfloat16)
        if self.fea_augment is not None and self.training:
            feats, _ = self.fea_augment(feats, wav_lens)
        feats = self.normalize(feats, wav_lens, epoch=epoch)
        x = self.enc(self.CNN(feats), wav_lens)
        return self.log_softmax(self.proj_ctc(self.proj_enc(x)).float())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=8.0)
    ap.add_argument("--augment", action="store_true", help="apply the recipe's fea_augment to the features")
    ap.add_argument("--wav-augment", action="store_true", help="apply the recipe's wav_augment (speed perturbation) to the waveforms")
    ap.add_argument("--decode", action="store_true", help="print the batch's CTC greedy hypotheses after the last step")
    ap.add_argument("--noam-warmup", type=int, default=0, metavar="N", help="Noam schedule on the device with N warm-up steps")
    ap.add_argument("--sgd-after", type=int, default=0, metavar="K", help="switch to Nesterov SGD (FlatSGD.adopt) after K steps")
    args = ap.parse_args()
    torch.manual_seed(0)
    model = EncoderSide(augment=args.augment, wav_augment=args.wav_augment).cuda().train()
    opt = FlatAdamW(model, lr=8e-4, betas=(0.9, 0.98), weight_decay=0.01, max_grad_norm=5.0, compute_dtype=torch.bfloat16)
    noam_annealing = None
    if args.noam_warmup > 0:
        noam_annealing = NoamScheduler(lr_initial=8e-4, n_warmup_steps=args.noam_warmup)
        opt.set_lr_schedule(noam_annealing)
    B, L = args.batch, int(16000 * args.seconds)
    wav = torch.randn(B, L, device="cuda") * 0.1
    wav_lens = torch.linspace(1.0, 0.6, B, device="cuda")
    for b in range(B):
        wav[b, int(L * float(wav_lens[b])):] = 0.0
    tokens = torch.randint(1, 1000, (B, 40), device="cuda")
    tok_lens = torch.ones(B, device="cuda")
    t0 = None
    for step in range(args.steps):
        if step == 3:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        opt.zero_grad()
        loss = ctc_loss(model(wav, wav_lens), tokens, wav_lens, tok_lens, blank_index=0)
        loss.backward()
        opt.step()
        if noam_annealing is not None:
            noam_annealing(opt)                # (attached: counts only; the device computed this update's rate)
        if step % 5 == 0 or step == args.steps - 1:
            print(f"step {step:3d}  ctc loss {loss.item():9.4f}" + (f"  lr {opt.current_lr():.3e}" if args.noam_warmup or args.sgd_after else ""))
        if args.sgd_after > 0 and step + 1 == args.sgd_after:
            opt = FlatSGD.adopt(opt, lr=1e-5, momentum=0.99, nesterov=True)     # lr_sgd of the AISHELL-1 recipe
            noam_annealing = None
            print(f"step {step:3d}  switched to Nesterov SGD over the same flat buffers")
    torch.cuda.synchronize()
    if t0 is not None and args.steps > 3:
        dt = (time.perf_counter() - t0) / (args.steps - 3)
        frames = B * (1 + L // 160 + 3) // 4
        print(f"{dt*1e3:.1f} ms/step, {frames/dt:,.0f} encoder frames/s including front-end and CTC head")
    if args.decode:
        model.eval()
        with torch.no_grad():
            hyps = ctc_greedy_decode(model(wav, wav_lens), wav_lens, blank_id=0)
        for b, h in enumerate(hyps):
            print(f"hyp {b:2d} ({len(h):3d} tokens): {' '.join(str(k) for k in h[:24])}{' ...' if len(h) > 24 else ''}")


if __name__ == "__main__":
    main()
