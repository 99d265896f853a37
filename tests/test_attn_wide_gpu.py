"""sdlt_attn_wide_fwd (one-pass attention for one wide head, csrc/attn_wide.hip) against softmax(scale Q K^T) V in float64 from the bf16-rounded inputs, at the
attention forward test's bar (tests/test_kernels_gpu.py: bf16 operands, fp32 scores, bf16 P, fp32 accumulation, one rounding), and the VAE / render built on it."""
import json
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _ref64(q, k, v, B, Nq, Nk, scale):
    q, k, v = (t.double().cpu() for t in (q, k, v))
    return torch.cat([torch.softmax(scale * q[b * Nq:(b + 1) * Nq] @ k[b * Nk:(b + 1) * Nk].T, dim=-1) @ v[b * Nk:(b + 1) * Nk] for b in range(B)])


@pytest.mark.parametrize("d,B,Nq,Nk,sharp,strided", [
    (512, 1, 1, 1, 1, False), (512, 1, 17, 17, 1, False), (512, 1, 64, 64, 1, False), (512, 2, 65, 65, 1, False), (512, 2, 200, 129, 1, False),
    (512, 1, 1032, 1032, 1, False), (128, 2, 128, 72, 1, False), (512, 1, 96, 96, 1, True), (512, 1, 300, 300, 8, False)])
def test_attn_wide_matches_fp64(d, B, Nq, Nk, sharp, strided):
    """sharp = 8: scale 8 / sqrt(d), a nearly one-hot softmax whose running maximum moves across the key tiles.  strided: q, k, v are column slices of one
    [N, 3 d] buffer.  Rows after O's last are a guard that must stay as filled; two runs must give the same bits."""
    from sd_lora_trainer_amd import ops
    g = torch.Generator().manual_seed(1000 * Nq + Nk + d)
    scale = sharp / math.sqrt(d)
    if strided:
        qkv = torch.randn(Nq, 3 * d, generator=g).to(BF16).cuda()
        q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    else:
        q, k, v = (torch.randn(B * n, d, generator=g).to(BF16).cuda() for n in (Nq, Nk, Nk))
    ref = _ref64(q, k, v, B, Nq, Nk, scale)
    assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0.1
    outs = []
    for _ in range(2):
        buf = torch.full((B * Nq + 8, d), 7.0, dtype=BF16, device="cuda")
        ops.attn_wide_fwd(q, k, v, buf[:B * Nq], B=B, Nq=Nq, Nk=Nk, scale=scale)
        torch.cuda.synchronize()
        assert bool((buf[B * Nq:] == 7.0).all()), "rows beyond B Nq were written"
        outs.append(buf[:B * Nq].clone())
    assert torch.equal(outs[0], outs[1]), "two runs differ"
    got = outs[0].double().cpu()
    err, bar = float((got - ref).abs().max()), 1.5e-2 * float(ref.abs().max()) + 1e-6
    print(f"attn_wide d={d} B={B} Nq={Nq} Nk={Nk} sharp={sharp}: max err {err:.3e} (bar {bar:.3e})")
    assert err <= bar
    if Nk == 1:
        assert torch.equal(outs[0], v[:1].expand(Nq, d)), "one key: O must be V's row"


def _cmp(a, b, what):
    a, b = a.float().cpu(), b.float().cpu()
    err = float((a - b).abs().max()) / float(b.abs().max())
    cos = float((a.reshape(-1).double() @ b.reshape(-1).double()) / (a.double().norm() * b.double().norm()))
    assert err <= 5e-2 and cos >= 0.995, (what, err, cos)


@pytest.mark.parametrize("kind,B,h,w", [("tiny", 2, 16, 8), ("tiny", 1, 9, 7), ("sd", 1, 32, 32)])
def test_vae_flash_matches_oracle(kind, B, h, w):
    """tests/test_vae_gpu.py's comparison and bars with attention="flash"; on the real topology also the peak memory of a first 64 x 64 decode: flash never
    allocates the fp32 scores [N, N] (N N 4 bytes = 67 MB at N = 4096), so its peak is lower by at least that."""
    from oracle import vae_ref as V
    from sd_lora_trainer_amd import vae
    import sd_lora_trainer_amd.unet as M
    cfg = V.CONFIGS[kind]
    sd = {k: v.to(BF16).float() for k, v in V.init_state(cfg, seed=0).items()}
    g = torch.Generator().manual_seed(1)
    z = torch.randn(B, 4, h, w, generator=g)
    rt = M.Runtime("cuda:0", B)
    dec, enc = vae.VaeDecoder(rt, sd, attention="flash"), vae.VaeEncoder(rt, sd, attention="flash")
    _cmp(dec.decode(z.cuda()), V.decode(cfg, sd, z), "decode")
    f = 2 ** (len(cfg["block_out_channels"]) - 1)
    x = torch.tanh(torch.randn(B, 3, f * h, f * w, generator=g))
    _cmp(enc.encode_moments(x.cuda()), V.encode_moments(cfg, sd, x), "encode moments")
    if kind == "sd":
        del dec, enc
        z64, peak = torch.randn(1, 4, 64, 64, generator=g).cuda(), {}
        for mode in ("flash", "dense"):
            d64 = vae.VaeDecoder(M.Runtime("cuda:0", 1), sd, attention=mode)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            d64.decode(z64)
            torch.cuda.synchronize()
            peak[mode] = torch.cuda.max_memory_allocated()
            del d64
        print(f"first 64 x 64 decode, peak bytes: {peak}")
        assert peak["dense"] - peak["flash"] >= 4096 * 4096 * 4, peak


def test_render_cli_vae_attention_flash(tmp_path, monkeypatch):
    """`render --vae-attention flash` on a one-step tinyxl job, with an init picture: the decoder and the encoder both run the kernel, prompts.json records it."""
    from PIL import Image
    from sd_lora_trainer_amd import ops, render as R, train as T
    from sd_lora_trainer_amd.config import TrainingConfig
    from tests.test_driver_cpu import _tokenizer_dir
    from tests.test_hires_gpu import _run
    monkeypatch.chdir(tmp_path)
    tok_dir, _ = _tokenizer_dir(tmp_path)
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", name="flash job", seed=3, resolution=256, train_batch_size=1, max_train_steps=1,
                         checkpointing_steps=1000, lora_rank=8, n_sample_imgs=0, output_dir=str(tmp_path / "job"),
                         pretrained_model={"path": "synthetic:tinyxl", "tokenizer_path": tok_dir})
    _, ckdir = _run(T.train(cfg))
    calls, real = [], ops.attn_wide_fwd
    monkeypatch.setattr(ops, "attn_wide_fwd", lambda *a, **k: (calls.append(k["Nq"]), real(*a, **k))[1])
    Image.new("RGB", (64, 64), (90, 140, 200)).save(tmp_path / "init.png")
    R.main(["--checkpoint", ckdir, "--out", str(tmp_path / "out"), "--prompt", "a photo of <concept>", "--size", "64", "64", "--steps", "4", "--seed", "11",
            "--init-image", str(tmp_path / "init.png"), "--vae-attention", "flash"])
    pics = list((tmp_path / "out").glob("img_00_seed11_scale*.jpg"))
    assert len(pics) == 1 and Image.open(pics[0]).size == (64, 64)
    assert json.load(open(tmp_path / "out" / "prompts.json"))["vae_attention"] == "flash"
    assert len(calls) == 2 and calls[0] == calls[1]          # one launch in the encoder, one in the decoder, at the same latent size
