"""sdlt_blur_planes on the MI355X against its contract in torch fp32 on the CPU (tests/blur_ref.py: the ordered sum), bit for bit."""
import pytest
import torch

from tests import blur_ref as BR

pytestmark = pytest.mark.gpu


def _planes(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


# 1 x 5 x 7 with sigma 2, 8: the radius (6, 24) reaches beyond the extent, every tap clamps; 3 x 33 x 70: two workgroups along x, a partial one along
# both axes, three planes (the 64-bit plane offset); sigma 0.5: R = 2
@pytest.mark.parametrize("clamp01", [False, True])
@pytest.mark.parametrize("shape,sigma", [((1, 5, 7), 2.0), ((1, 5, 7), 8.0), ((3, 33, 70), 0.5), ((3, 33, 70), 2.0), ((3, 33, 70), 8.0)])
def test_blur_planes_exact(shape, sigma, clamp01):
    from sd_lora_trainer_amd import ops
    taps = ops.blur_taps(sigma)
    src = _planes(shape, 11)
    if clamp01:                                           # a third of the plane below 0 and a third above 1: the clamp has something to do
        src = src * 0.2
        src[..., : shape[2] // 3] -= 0.6
        src[..., -(shape[2] // 3):] += 1.3
    ref = BR.blur_planes(src, torch.empty(shape), torch.empty(shape), taps, clamp01)
    if clamp01 and shape[2] == 70:
        assert float(ref.min()) == 0.0 and float(ref.max()) == 1.0
        assert not torch.equal(ref, BR.blur_planes(src, torch.empty(shape), torch.empty(shape), taps, False))
    d_src, d_taps = src.cuda(), taps.cuda()
    out, scratch = torch.full(shape, float("nan"), device="cuda"), torch.full(shape, float("nan"), device="cuda")
    assert ops.blur_planes(d_src, out, scratch, d_taps, clamp01) is out
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref), int((out.cpu() != ref).sum())
    assert torch.equal(d_src.cpu(), src)                                                          # the input is not touched
    inplace = d_src.clone()
    ops.blur_planes(inplace, inplace, scratch, d_taps, clamp01)                                  # out == in
    assert torch.equal(inplace.cpu(), ref)


def test_impulse_stays_symmetric_and_constant_stays_close():
    from sd_lora_trainer_amd import ops
    taps = ops.blur_taps(2.0).cuda()
    imp = torch.zeros(1, 33, 35, device="cuda")
    imp[0, 16, 17] = 1.0
    out = ops.blur_planes(imp, torch.empty_like(imp), torch.empty_like(imp), taps).cpu()
    assert torch.equal(out, out.flip(1)) and torch.equal(out, out.flip(2)) and float(out[0, 16, 17]) == float(out.max())
    t = taps.cpu()
    assert torch.equal(out[0, 10:23, 11:24], t[:, None] * t[None, :])                             # one product per sample: the outer product of the taps
    assert abs(float(out.double().sum()) - 1.0) < 1e-5


def test_refusals():
    from tests.test_diffdiff_cpu import test_blur_entry_point_validation
    test_blur_entry_point_validation()
    from sd_lora_trainer_amd import _lib, ops
    x = torch.zeros(1, 5, 7, device="cuda")
    with pytest.raises(_lib.KernelLibraryError, match="scratch overlaps"):
        ops.blur_planes(x, torch.empty_like(x), x, ops.blur_taps(1.0).cuda())
    torch.cuda.synchronize()
