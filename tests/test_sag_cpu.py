"""Self-attention guidance without a GPU: sampler.sag_table, every refusal of LatentSampler.sample(sag=) before the UNet is touched, the unchanged
Trajectory, and the command line's defaults."""
import unittest.mock as mock

import pytest
import torch

from sd_lora_trainer_amd import sampler as SM
from tests import multistep_ref as MR
from tests.test_multistep_cpu import EMB, _Stub
import sd_lora_trainer_amd.unet as unet_mod

launched = lambda *a, **k: pytest.fail("launched")  # noqa: E731
SAG_OPS = dict(attn_colmass=launched, sag_degrade=launched, sag_apply=launched)


def test_sag_table():
    s = SM.EulerDiscrete().set_timesteps(4)
    tab = SM.sag_table(s, True)
    assert tuple(tab.shape) == (5, 4) and tab.dtype == torch.float32 and tab[0].tolist() == [4.0, 0.0, 0.0, 0.0]
    assert torch.equal(tab[1:, 0], torch.from_numpy(s.sigmas[:4])) and tab[1:, 1:].tolist() == [[0.5, 1.0, 0.0]] * 4 and SM.SAG_DEFAULT == (0.5, 2.0, 1.0)
    tab = SM.sag_table(s, dict(scale=[0.1, 0.2, 0.3], threshold=1.25), k=3)
    assert tab[0, 0] == 3 and tab[1:, 1].tolist() == pytest.approx([0.1, 0.2, 0.3]) and tab[1:, 2].tolist() == [1.25] * 3
    with pytest.raises(ValueError, match=r"3 scale\(s\) for the 4 step"):
        SM.sag_table(s, ([0.1, 0.2, 0.3], 2.0, 1.0))
    assert SM.sag_args(None) is None and SM.sag_args(False) is None and SM.sag_args((1, 3, 0.5)) == (1.0, 3.0, 0.5)


def _stub(pred="epsilon", ops=SAG_OPS):
    rt = unet_mod.Runtime("cpu", 2, act_dtype=torch.float32, ops=type("T", (), {**vars(MR.emu_ms), **ops}))
    stub = _Stub(8, 8, 7)
    return SM.LatentSampler(rt, stub, prediction_type=pred), stub


@pytest.mark.parametrize("pred,ops,kw,exc,msg", [
    ("v_prediction", SAG_OPS, dict(sag=True), NotImplementedError, "v_prediction"),
    ("epsilon", {}, dict(sag=True), NotImplementedError, "sdlt_attn_colmass"),
    ("epsilon", SAG_OPS, dict(sag=True, tile=4), ValueError, "sag does not combine with tile"),
    ("epsilon", SAG_OPS, dict(sag=True, regions=dict(masks=None, embeds=[])), ValueError, "sag does not combine with regions"),
    ("epsilon", SAG_OPS, dict(sag=True, heatmap=dict(cols=[[1]])), ValueError, "sag does not combine with heatmap"),
    ("epsilon", SAG_OPS, dict(sag=(-0.5, 2.0, 1.0)), ValueError, "scale"), ("epsilon", SAG_OPS, dict(sag=(float("inf"), 2.0, 1.0)), ValueError, "scale"),
    ("epsilon", SAG_OPS, dict(sag=(0.5, 0.0, 1.0)), ValueError, "blur_sigma"), ("epsilon", SAG_OPS, dict(sag=(0.5, float("nan"), 1.0)), ValueError, "blur_sigma"),
    ("epsilon", SAG_OPS, dict(sag=dict(blur=2.0)), ValueError, "unknown"), ("epsilon", SAG_OPS, dict(sag=(0.5, 2.0)), ValueError, "sag takes")])
@pytest.mark.parametrize("fused", [False, True])
def test_refused_before_anything_is_built(fused, pred, ops, kw, exc, msg):
    smp, stub = _stub(pred, ops)
    with pytest.raises(exc, match=msg):
        smp.sample(EMB, 8, 8, steps=3, latents=torch.zeros(1, 4, 8, 8), fused=fused, **kw)
    assert stub.calls == 0 and smp._fused is None and smp._sag is None


@pytest.mark.parametrize("kw,name", [(dict(kv_downsample=(1, 1, 2)), "kv_downsample"), (dict(hypertile=dict(tile=1, depth=2)), "hypertile"),
                                     (dict(token_merge=dict(ratio=0.5, depth=2)), "token_merge")])
def test_refused_at_a_depth_that_reaches_the_mid_block(kw, name):
    from oracle import unet_ref as U
    from tests.test_tilediff_cpu import _embeds
    from tests.test_tome_cpu import _unet
    unet = _unet(True)
    unet.rt.ops = type("T", (unet.rt.ops,), SAG_OPS)
    with pytest.raises(ValueError, match=f"sag does not combine with {name} at a depth that reaches the mid block's 4 x 4 token grid"):
        SM.LatentSampler(unet.rt, unet).sample(_embeds(U.CONFIGS["tiny15"], 5, 1)[0], 16, 16, steps=2, sag=True, **kw)
    assert unet._kv_ds is None and unet._ht is None and unet._tome is None and not unet._probe and unet.probe_layer().probed is None      # the UNet is untouched
    unet = _unet(True)
    unet.set_attention_probe(True)
    with pytest.raises(NotImplementedError, match="attention probe is an inference option"):
        unet.forward(torch.zeros(2 * 64, 64), torch.zeros(2), torch.zeros(2 * unet_mod.CTX_PAD, unet.cfg["cross_dim"]), B=2, H=8, W=8)


def test_trajectory_is_unchanged():
    assert SM.Trajectory._fields[-1] == "dyn" and "sag" not in SM.Trajectory._fields


def test_cli_defaults(tmp_path, capsys):
    from sd_lora_trainer_amd import render as R
    base, seen = ["--checkpoint", str(tmp_path / "nowhere"), "--out", str(tmp_path / "out")], {}
    with mock.patch.object(R, "load_for_inference", lambda *a, **k: "loaded"), mock.patch.object(R, "render", lambda loaded, prompts, out, **kw: seen.update(kw) or {}):
        R.main(base)
        assert "sag" not in seen
        R.main(base + ["--sag"])
        assert (seen["sag"], seen["sag_blur"], seen["sag_threshold"]) == (0.5, 2.0, 1.0)
        R.main(base + ["--sag", "0.8", "--sag-threshold", "1.2"])
        assert (seen["sag"], seen["sag_blur"], seen["sag_threshold"]) == (0.8, 2.0, 1.2)
    for extra, msg in ((["--sag-blur", "3"], "need sag"), (["--sag", "--sag-blur", "0"], "blur_sigma"), (["--sag", "--heatmap", "cat"], "--heatmap")):
        with pytest.raises(SystemExit):
            R.main(base + extra)
        assert msg in capsys.readouterr().err
