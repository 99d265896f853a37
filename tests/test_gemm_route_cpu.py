"""Which tiled-GEMM kernel a call runs, pinned without a GPU: sdlt_gemm_route is the host-side plan of sdlt_gemm_bf16 (gemm_validate / gemm_plan in
csrc/gemm.hip) and launches nothing.  The bit-exact parity files compare numbers only, so a threshold edit that moves a shape of the workload onto
another tile, ring depth or split passes them; this file is what notices.  Every expected value below was recorded from the dispatcher as it stood
before gemm_plan existed (its launch<...> patched to record its template arguments instead of launching), never from gemm_plan itself.
A route is (tile, ring depth, splitk, variant); the addresses are made up and 256-byte aligned: nothing dereferences them."""
import ctypes

import pytest

from sd_lora_trainer_amd import _lib

ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED = -1, -2, -4      # csrc/common.h
BASE = 0x10000000


def block(M, N, K, *, conv=False, rank=0, ws=True, **over):
    """The parameter block of an [M, K] x [N, K]^T product (conv: the 3x3 convolution form, K = 9 Cin) with a padded adapter rank and a split-K workspace."""
    p = _lib.GemmParams()
    p.X, p.W, p.C = BASE, BASE + 0x100, BASE + 0x200
    p.M, p.N, p.K = M, N, K
    p.ldx, p.ldw, p.ldc = K, K, N
    p.alpha = 1.0
    if conv:
        side = next(s for s in (128, 64, 32, 16, 8, 4, 2, 1) if M % (s * s) == 0)
        p.mode, p.zero, p.Cin, p.stride = 1, BASE + 0x300, K // 9, 1
        p.Hin = p.Win = p.Hout = p.Wout = side
        p.ldx = p.Cin
    if rank:
        p.lora_R, p.lora_scale = rank, 1.0
        p.Adown, p.Bup, p.T_out = BASE + 0x600, BASE + 0x700, BASE + 0x800
        p.ld_adown, p.ld_bup, p.ld_t = K, rank, rank
    if ws:
        p.ws_slab, p.ws_slab_bytes, p.ws_cnt, p.ws_cnt_len = BASE + 0x1000, 1 << 30, BASE + 0x2000, 1 << 20
    for k, v in over.items():
        setattr(p, k, v)
    return p


def seg2(K2=64, **over):
    """Options of a second K segment."""
    return dict(K2=K2, X2=BASE + 0x400, W2=BASE + 0x500, ldx2=K2, ldw2=K2, **over)


def epi(op):
    """Options of a fused epilogue (1 GEGLU forward, 2 GEGLU backward, 3 activation side output, 4 activation backward)."""
    return dict(epi_op=op, epi_out=BASE + 0x4000, ld_epi_out=16384, epi_in=BASE + 0x5000, ld_epi_in=16384)


def ln(parts=0):
    """Options of a folded LayerNorm, with `parts` producer partials per row."""
    return dict(ln_c1=BASE + 0x6000, ln_adapter=BASE + 0x6100, ln_stats=BASE + 0x6200, ln_eps=1e-5, ln_parts=BASE + 0x6300 if parts else 0, ln_nparts=parts)


def plan(p):
    """The GemmPlan of block p, or the negative error code."""
    pl = _lib.GemmPlan()
    rc = _lib.load().sdlt_gemm_route(ctypes.byref(p), ctypes.byref(pl))
    return rc if rc else pl


def route(p):
    pl = plan(p)
    return pl if isinstance(pl, int) else (pl.tile, pl.stages, pl.splitk, _lib.gemm_variant(pl))


def refusal(p):
    """(code, message) of a refused block - and the launch entry refuses it alike, before it touches the device."""
    lib = _lib.load()
    rc = route(p)
    assert isinstance(rc, int) and rc < 0, rc
    msg = lib.sdlt_last_error().decode()
    assert lib.sdlt_gemm_bf16(ctypes.byref(p), None) == rc and lib.sdlt_last_error().decode() == msg
    return rc, msg


# ---------------------------------------------------------------------------------------------- 1. the workload's products at default options
# (label, M, N, K, conv): the shapes the planner's comments quote, and the text encoders' (M = 128)
WORKLOAD = [
    ("ff.net.0.proj 1024 x 10240 x 1280", 1024, 10240, 1280, False),
    ("ff.net.0.proj / ff.net.2 1024 x 5120 x 1280", 1024, 5120, 1280, False),
    ("ff.net.0.proj 4096 x 2560 x 640 (hidden half)", 4096, 2560, 640, False),
    ("to_q|to_k|to_v 4096 x 1920 x 640", 4096, 1920, 640, False),
    ("attention projection 1024 x 1280 x 1280", 1024, 1280, 1280, False),
    ("conv 16384 x 320, K 2880", 16384, 320, 2880, True),
    ("conv 16384 x 320, K 8640", 16384, 320, 8640, True),
    ("conv 4096 x 640, K 2880", 4096, 640, 2880, True),
    ("conv 4096 x 640, K 5760", 4096, 640, 5760, True),
    ("conv 4096 x 640, K 11520", 4096, 640, 11520, True),
    ("conv 256 x 1280, K 11520", 256, 1280, 11520, True),
    ("ff.net.2 256 x 1280 x 5120", 256, 1280, 5120, False),
    ("CLIP-L out_proj 128 x 768 x 768", 128, 768, 768, False),
    ("CLIP-L fc2 128 x 768 x 3072", 128, 768, 3072, False),
    ("CLIP-L qkv 128 x 2304 x 768", 128, 2304, 768, False),
    ("CLIP-L fc1 128 x 3072 x 768", 128, 3072, 768, False),
]
OPTIONS = [(rank, ws, hint) for rank in (0, 16) for ws in (False, True) for hint in (0, 1)]
# per shape, in OPTIONS order (no adapter: no workspace, + throughput_hint, workspace, + throughput_hint; then the same with a rank-16 adapter):
# (tile, ring depth, splitk), all of the PLAIN variant
DEFAULT = {
    'ff.net.0.proj 1024 x 10240 x 1280': [(7, 3, 1), (4, 3, 1), (7, 3, 1), (4, 3, 1), (2, 2, 1), (4, 3, 1), (2, 2, 1), (4, 3, 1)],
    'ff.net.0.proj / ff.net.2 1024 x 5120 x 1280': [(8, 4, 1), (4, 3, 1), (8, 4, 1), (4, 3, 1), (2, 2, 1), (4, 3, 1), (2, 2, 1), (4, 3, 1)],
    'ff.net.0.proj 4096 x 2560 x 640 (hidden half)': [(7, 3, 1), (4, 3, 1), (7, 3, 1), (4, 3, 1), (1, 2, 1), (4, 3, 1), (1, 2, 1), (4, 3, 1)],
    'to_q|to_k|to_v 4096 x 1920 x 640': [(8, 4, 1), (4, 3, 1), (8, 4, 1), (4, 3, 1), (1, 2, 1), (4, 3, 1), (1, 2, 1), (4, 3, 1)],
    'attention projection 1024 x 1280 x 1280': [(2, 4, 1), (2, 4, 1), (2, 4, 1), (2, 4, 1), (2, 4, 1), (2, 4, 1), (2, 4, 1), (2, 4, 1)],
    'conv 16384 x 320, K 2880': [(8, 4, 1), (4, 3, 1), (8, 4, 1), (4, 3, 1), (8, 4, 1), (4, 3, 1), (8, 4, 1), (4, 3, 1)],
    'conv 16384 x 320, K 8640': [(8, 4, 1), (4, 3, 1), (8, 4, 1), (4, 3, 1), (8, 4, 1), (4, 3, 1), (8, 4, 1), (4, 3, 1)],
    'conv 4096 x 640, K 2880': [(1, 2, 1), (4, 3, 1), (8, 4, 2), (4, 3, 3), (1, 2, 1), (4, 3, 1), (8, 4, 2), (4, 3, 3)],
    'conv 4096 x 640, K 5760': [(1, 2, 1), (4, 3, 1), (8, 4, 2), (4, 3, 3), (1, 2, 1), (4, 3, 1), (8, 4, 2), (4, 3, 3)],
    'conv 4096 x 640, K 11520': [(1, 2, 1), (4, 3, 1), (8, 4, 2), (4, 3, 3), (1, 2, 1), (4, 3, 1), (8, 4, 2), (4, 3, 3)],
    'conv 256 x 1280, K 11520': [(2, 4, 1), (2, 4, 1), (2, 4, 6), (2, 4, 6), (2, 4, 1), (2, 4, 1), (2, 4, 6), (2, 4, 6)],
    'ff.net.2 256 x 1280 x 5120': [(2, 4, 1), (2, 4, 1), (2, 4, 4), (2, 4, 4), (2, 4, 1), (2, 4, 1), (2, 4, 4), (2, 4, 4)],
    'CLIP-L out_proj 128 x 768 x 768': [(3, 4, 1), (3, 4, 1), (3, 4, 3), (3, 4, 3), (3, 4, 1), (3, 4, 1), (3, 4, 3), (3, 4, 3)],
    'CLIP-L fc2 128 x 768 x 3072': [(3, 4, 1), (3, 4, 1), (3, 4, 4), (3, 4, 4), (3, 4, 1), (3, 4, 1), (3, 4, 4), (3, 4, 4)],
    'CLIP-L qkv 128 x 2304 x 768': [(3, 4, 1), (3, 4, 1), (3, 4, 1), (3, 4, 1), (3, 4, 1), (3, 4, 1), (3, 4, 1), (3, 4, 1)],
    'CLIP-L fc1 128 x 3072 x 768': [(3, 4, 1), (3, 4, 1), (3, 4, 1), (3, 4, 1), (3, 4, 1), (3, 4, 1), (3, 4, 1), (3, 4, 1)],
}


def test_workload_routes_at_default_options():
    assert len(DEFAULT) == len(WORKLOAD)
    for label, M, N, K, conv in WORKLOAD:
        got = [route(block(M, N, K, conv=conv, rank=rank, ws=ws, throughput_hint=hint)) for rank, ws, hint in OPTIONS]
        assert got == [r + ("PLAIN",) for r in DEFAULT[label]], label


# ---------------------------------------------------------------------------------------------- 2. both sides of every threshold, the re-maps, the variants
# (what, block, route)
PINNED = [
    # t128 = ceil(M / 128) ceil(N / 128) at 160: 64x128 tiles below, 128x128 with the deep ring from there
    ('t128 159, K 1280', block(384, 6784, 1280), (2, 4, 1, 'PLAIN')),
    ('t128 160, K 1280', block(512, 5120, 1280), (1, 4, 1, 'PLAIN')),
    # t128 at 320: the deep 128x128 tile below; 256x128 without an adapter, the shallow ring with one
    ('t128 319', block(1408, 3712, 1280), (1, 4, 1, 'PLAIN')),
    ('t128 320', block(1280, 4096, 1280), (4, 3, 1, 'PLAIN')),
    ('t128 512, N 1024', block(8192, 1024, 1280), (4, 3, 1, 'PLAIN')),
    ('t128 512, N 896', block(9472, 896, 1280), (2, 2, 1, 'PLAIN')),
    ('t128 520', block(1280, 6656, 1280), (2, 2, 1, 'PLAIN')),
    ('t128 319, adapter', block(1408, 3712, 1280, rank=16), (1, 4, 1, 'PLAIN')),
    ('t128 320, adapter', block(1280, 4096, 1280, rank=16), (2, 2, 1, 'PLAIN')),
    # 160-column tiles: t8 = ceil(M / 128) N / 160 at 224, t7 = ceil(M / 256) N / 160 at 256, K at 2560
    ('t8 222', block(768, 5920, 1280), (1, 4, 1, 'PLAIN')),
    ('t8 224', block(896, 5120, 1280), (8, 4, 1, 'PLAIN')),
    ('t7 255', block(768, 13600, 1280), (8, 4, 1, 'PLAIN')),
    ('t7 256', block(1024, 10240, 1280), (7, 3, 1, 'PLAIN')),
    ('t7 256, K 2560', block(1024, 10240, 2560), (7, 3, 1, 'PLAIN')),
    ('t7 256, K 2624', block(1024, 10240, 2624), (2, 2, 1, 'PLAIN')),
    ('t7 256, M 128', block(128, 40960, 1280), (3, 4, 1, 'PLAIN')),
    ('t7 256, throughput_hint', block(1024, 10240, 1280, throughput_hint=1), (4, 3, 1, 'PLAIN')),
    ('t7 256, rank pad 32', block(1024, 10240, 1280, rank=32), (2, 2, 1, 'PLAIN')),
    # ... with a rank-16 adapter: K <= 640 and 224 <= t8 <= 320
    ('adapter, t8 256, K 640', block(4096, 1280, 640, rank=16), (8, 4, 1, 'PLAIN')),
    ('adapter, t8 256, K 704', block(4096, 1280, 704, rank=16), (2, 2, 1, 'PLAIN')),
    ('adapter, t8 216, K 640', block(1024, 4320, 640, rank=16), (1, 4, 1, 'PLAIN')),
    ('adapter, t8 320, K 640', block(4096, 1600, 640, rank=16), (8, 4, 1, 'PLAIN')),
    ('adapter, t8 328, K 640', block(5248, 1280, 640, rank=16), (1, 2, 1, 'PLAIN')),
    ('adapter, t8 256, K 640, lora_group_n', block(4096, 1280, 640, rank=16, lora_group_n=640), (1, 2, 1, 'PLAIN')),
    # ... convolutions: t8 of 256, 128 or 64, split to 256 workgroups while every split keeps 16 K steps
    ('conv, t8 256', block(16384, 320, 2880, conv=True), (8, 4, 1, 'PLAIN')),
    ('conv, t8 128, 22 steps per split', block(4096, 640, 2880, conv=True), (8, 4, 2, 'PLAIN')),
    ('conv, t8 128, 13 steps per split', block(4096, 640, 1728, conv=True), (3, 2, 1, 'PLAIN')),
    ('conv, t8 64, 18 steps per split', block(4096, 320, 4608, conv=True), (8, 4, 4, 'PLAIN')),
    ('conv, t8 64, 15 steps per split', block(4096, 320, 4032, conv=True), (1, 4, 3, 'PLAIN')),
    ('conv, t8 128, no workspace', block(4096, 640, 2880, conv=True, ws=False), (1, 2, 1, 'PLAIN')),
    ('conv, t8 128, forced splitk 1', block(4096, 640, 2880, conv=True, splitk=1), (1, 2, 1, 'PLAIN')),
    ('conv + second segment, t8 256', block(16384, 320, 2880, conv=True, **seg2()), (8, 4, 1, 'PLAIN')),
    # t128 >= 320 with an adapter: K at 640
    ('adapter, t128 352, K 640', block(4096, 1408, 640, rank=16), (1, 2, 1, 'PLAIN')),
    ('adapter, t128 352, K 704', block(4096, 1408, 704, rank=16), (2, 2, 1, 'PLAIN')),
    ('adapter, t128 352, K 704, stages 4', block(4096, 1408, 704, rank=16, stages=4), (2, 4, 1, 'PLAIN')),
    # 160 <= t128 < 320: K at 6144 for a product, at 2560 for a convolution
    ('t128 192, K 6144', block(4096, 704, 6144), (1, 4, 1, 'PLAIN')),
    ('t128 192, K 6208', block(4096, 704, 6208), (1, 2, 3, 'PLAIN')),
    ('t128 192, K 6208, no workspace', block(4096, 704, 6208, ws=False), (1, 2, 1, 'PLAIN')),
    ('t128 192, K 1536 + 64 in a second segment', block(4096, 704, 1536, **seg2()), (1, 4, 1, 'PLAIN')),
    ('conv, t128 192, K 2304', block(4096, 704, 2304, conv=True), (3, 2, 1, 'PLAIN')),
    ('conv, t128 192, K 2880', block(4096, 704, 2880, conv=True), (1, 2, 3, 'PLAIN')),
    ('conv + second segment, t128 192, K 1152 + 1472', block(4096, 704, 1152, conv=True, **seg2(K2=1472)), (1, 2, 3, 'PLAIN')),
    ('conv, t128 192, throughput_hint', block(4096, 704, 2880, conv=True, throughput_hint=1), (4, 3, 3, 'PLAIN')),
    ('t128 192, throughput_hint', block(4096, 704, 1280, throughput_hint=1), (1, 4, 1, 'PLAIN')),
    ('t128 320, throughput_hint, adapter', block(1280, 4096, 1280, rank=16, throughput_hint=1), (4, 3, 1, 'PLAIN')),
    # t128 < 160: K at 2560, t128 at 32 (the unsplit 64x128 tile above) and at 24 (the long-K split of the 64x128 tile)
    ('t128 36, K 2560', block(512, 1152, 2560), (2, 4, 1, 'PLAIN')),
    ('t128 32, K 2560', block(512, 1024, 2560), (2, 4, 4, 'PLAIN')),
    ('t128 36, K 2624', block(512, 1152, 2624), (1, 4, 5, 'PLAIN')),
    ('t128 24, K 5120', block(256, 1536, 5120), (2, 4, 4, 'PLAIN')),
    ('t128 26, K 5120', block(256, 1664, 5120), (1, 4, 10, 'PLAIN')),
    ('t128 24, K 5120, fp32 output', block(256, 1536, 5120, out_fp32=1), (1, 4, 11, 'PLAIN')),
    ('t128 20, K 5120, adapter', block(256, 1280, 5120, rank=16), (2, 4, 4, 'PLAIN')),
    ('t128 20, K 3840: 20 steps per split', block(256, 1280, 3840), (2, 4, 3, 'PLAIN')),
    # M <= 128: 64x64 tiles; no split from 100 tiles, three from 60 when K has 24 steps, four below, never under 4 steps per split
    ('M 128, 100 tiles', block(128, 3200, 1536), (3, 4, 1, 'PLAIN')),
    ('M 128, 98 tiles, 24 steps', block(128, 3136, 1536), (3, 4, 3, 'PLAIN')),
    ('M 128, 98 tiles, 23 steps', block(128, 3136, 1472), (3, 4, 1, 'PLAIN')),
    ('M 128, 60 tiles, 24 steps', block(128, 1920, 1536), (3, 4, 3, 'PLAIN')),
    ('M 128, 58 tiles, 24 steps', block(128, 1856, 1536), (3, 4, 4, 'PLAIN')),
    ('M 128, 58 tiles, 12 steps', block(128, 1856, 768), (3, 4, 3, 'PLAIN')),
    ('M 128, 58 tiles, 4 steps', block(128, 1856, 256), (3, 4, 1, 'PLAIN')),
    ('M 129, 58 tiles of 64 x 64', block(129, 1856, 1536), (2, 4, 3, 'PLAIN')),
    ('M 64, N 65', block(64, 65, 1536), (2, 4, 8, 'PLAIN')),
    ('M 64, N 64', block(64, 64, 1536), (3, 4, 8, 'PLAIN')),
    ('M 1024, N 64', block(1024, 64, 1536), (3, 4, 8, 'PLAIN')),
    # the generic K split of a forced tile: up to 96 tiles, 8 steps per split (3 up to 32 tiles), 16 splits at most
    ('forced tile 1, 96 tiles', block(1024, 1536, 1536, tile=1), (1, 4, 3, 'PLAIN')),
    ('forced tile 1, 104 tiles', block(1024, 1664, 1536, tile=1), (1, 4, 1, 'PLAIN')),
    ('forced tile 1, 32 tiles, 20 steps', block(512, 1024, 1280, tile=1), (1, 4, 6, 'PLAIN')),
    ('forced tile 1, 33 tiles, 20 steps', block(384, 1408, 1280, tile=1), (1, 4, 2, 'PLAIN')),
    ('forced tile 1, 1 tile, 100 steps', block(128, 128, 6400, tile=1), (1, 4, 16, 'PLAIN')),
    ('forced tile 1, 1 tile, 2 steps', block(128, 128, 128, tile=1), (1, 4, 1, 'PLAIN')),
    ('forced tile 1, 96 tiles, no workspace', block(1024, 1536, 1536, tile=1, ws=False), (1, 4, 1, 'PLAIN')),
    ('forced tile 7, stages 2', block(1024, 10240, 1280, tile=7, stages=2, splitk=1), (7, 2, 1, 'PLAIN')),
    ('forced tile 6, rank pad 32', block(1024, 1024, 1280, rank=32, tile=6, splitk=1), (6, 2, 1, 'PLAIN')),
    ('forced tile 5, rank pad 64', block(1024, 1024, 1280, rank=64, tile=5, splitk=1), (5, 3, 1, 'PLAIN')),
    ('forced tile 4, rank pad 64, stages 2', block(1024, 1024, 1280, rank=64, tile=4, splitk=1, stages=2), (4, 2, 1, 'PLAIN')),
    # column groups: 64-wide groups move an unforced call to the 64x64 tile, wider ones stay
    ('lora_group_n 64, tile 0', block(1024, 1920, 640, rank=16, lora_group_n=64), (3, 4, 1, 'PLAIN')),
    ('lora_group_n 640, tile 0', block(4096, 1920, 640, rank=16, lora_group_n=640), (1, 2, 1, 'PLAIN')),
    ('lora_group_n 128, forced tile 2', block(1024, 1920, 640, rank=16, lora_group_n=128, tile=2, splitk=1), (2, 4, 1, 'PLAIN')),
    ('x2_group_n 64, tile 0', block(1024, 1920, 640, **seg2(x2_group_n=64)), (3, 4, 1, 'PLAIN')),
    ('x2_group_n 128, forced tile 1', block(1024, 1920, 640, tile=1, splitk=1, **seg2(x2_group_n=128)), (1, 4, 1, 'PLAIN')),
    # K-grouped adapters: 128x128 from 64 tiles of it, what the heuristics chose (1..3) below; one split per group or none
    ('lora_group_k, t128 64', block(1024, 1024, 1280, rank=16, lora_group_k=640), (1, 4, 2, 'KGROUP')),
    ('lora_group_k, t128 56', block(1024, 896, 1280, rank=16, lora_group_k=640), (2, 4, 2, 'KGROUP')),
    ('lora_group_k, t128 160 x 2 groups', block(4096, 640, 1280, rank=16, lora_group_k=640), (1, 4, 2, 'KGROUP')),
    ('lora_group_k, t128 165 x 2 groups', block(4224, 640, 1280, rank=16, lora_group_k=640), (1, 4, 1, 'KGROUP')),
    ('lora_group_k, no workspace', block(1024, 1024, 1280, rank=16, lora_group_k=640, ws=False), (1, 4, 1, 'KGROUP')),
    ('lora_group_k, one group', block(1024, 1024, 1280, rank=16, lora_group_k=1280), (1, 4, 1, 'KGROUP')),
    ('lora_group_k, forced splitk G', block(4224, 640, 1920, rank=32, lora_group_k=640, splitk=3), (1, 3, 3, 'KGROUP')),
    ('lora_group_k, forced splitk G + 1', block(4224, 640, 1920, rank=32, lora_group_k=640, splitk=4), (1, 3, 1, 'KGROUP')),
    ('lora_group_k, forced tile 3, rank pad 64', block(1024, 1024, 1280, rank=64, lora_group_k=320, tile=3), (3, 4, 4, 'KGROUP')),
    # batched launches: no split, whatever is asked
    ('batched', block(154, 1280, 2048, batch=BASE + 0x3000, n_batch=70), (2, 4, 1, 'BATCH')),
    ('batched, forced splitk 4, adapter', block(154, 1280, 2048, rank=16, batch=BASE + 0x3000, n_batch=65535, splitk=4, tile=3), (3, 4, 1, 'BATCH')),
    ('batched, K groups', block(154, 2048, 2560, rank=16, lora_group_k=1280, batch=BASE + 0x3000, n_batch=2), (2, 4, 1, 'KGROUP_BATCH')),
    # fused epilogues: tiles 4 / 5 / 6 move to 1, the deep ring whatever is asked
    ('GEGLU forward 1024 x 10240 x 1280', block(1024, 10240, 1280, **epi(1)), (7, 3, 1, 'EPI1')),
    ('GEGLU forward, throughput_hint: 256x128 moves to 128x128', block(4096, 5120, 640, throughput_hint=1, **epi(1)), (1, 4, 1, 'EPI1')),
    ('GEGLU backward 1024 x 5120 x 1280', block(1024, 5120, 1280, **epi(2)), (8, 4, 1, 'EPI2')),
    ('activation side output, M 128', block(128, 3072, 768, **epi(3)), (3, 4, 1, 'EPI3')),
    ('activation backward, forced tile 5, stages 2', block(128, 768, 3072, tile=5, stages=2, splitk=1, **epi(4)), (1, 4, 1, 'EPI4')),
    # folded LayerNorm: no split; an adapter on tiles 1, 2, 3, 8 (others: 1, or 3 under adapter groups no multiple of 128), GEGLU on 1, 2, 3, 7, 8
    ('LayerNorm + adapter 1024 x 1280 x 1280', block(1024, 1280, 1280, rank=16, **ln()), (2, 4, 1, 'LN_ADAPTER')),
    ('LayerNorm + adapter, partials', block(1024, 1280, 1280, rank=16, **ln(16)), (2, 4, 1, 'LN_ADAPTER_PARTS')),
    ('LayerNorm + adapter, partials, stages 2', block(1024, 1280, 1280, rank=16, stages=2, **ln(16)), (2, 2, 1, 'LN_ADAPTER')),
    ('LayerNorm + adapter, 17 partials', block(1024, 1280, 1280, rank=16, **ln(17)), (2, 4, 1, 'LN_ADAPTER')),
    ('LayerNorm + adapter, 3 partials', block(1024, 1280, 1280, rank=16, **ln(3)), (2, 4, 1, 'LN_ADAPTER')),
    ('LayerNorm + adapter, partials, 64x64 tile', block(1024, 1280, 1280, rank=16, tile=3, **ln(16)), (3, 4, 1, 'LN_ADAPTER')),
    ('LayerNorm + adapter, t8 256', block(4096, 1280, 640, rank=16, **ln()), (8, 4, 1, 'LN_ADAPTER')),
    ('LayerNorm + adapter, forced tile 4', block(1024, 1280, 1280, rank=16, tile=4, **ln()), (1, 4, 1, 'LN_ADAPTER')),
    ('LayerNorm + adapter, forced tile 7, 320-wide groups', block(1024, 1280, 1280, rank=16, tile=7, lora_group_n=320, **ln()), (3, 4, 1, 'LN_ADAPTER')),
    ('LayerNorm + adapter, 4 tiles: no split', block(128, 256, 1280, rank=16, tile=1, **ln()), (1, 4, 1, 'LN_ADAPTER')),
    ('LayerNorm + GEGLU 1024 x 10240 x 1280', block(1024, 10240, 1280, **ln(), **epi(1)), (7, 3, 1, 'LN_GEGLU')),
    ('LayerNorm + GEGLU, partials', block(1024, 10240, 1280, **ln(16), **epi(1)), (7, 3, 1, 'LN_GEGLU_PARTS')),
    ('LayerNorm + GEGLU, partials, 128x160 tile', block(1024, 5120, 1280, **ln(16), **epi(1)), (8, 4, 1, 'LN_GEGLU')),
    ('LayerNorm + GEGLU, forced tile 6, stages 2', block(1024, 5120, 1280, tile=6, stages=2, **ln(), **epi(1)), (1, 4, 1, 'LN_GEGLU')),
]


@pytest.mark.parametrize("what,p,want", PINNED, ids=[c[0] for c in PINNED])
def test_pinned_route(what, p, want):
    assert route(p) == want


def test_every_variant_is_reached():
    assert {want[3] for _, _, want in PINNED} == set(_lib.GEMM_VARIANTS.values()), "a variant no case reaches"


def test_plan_fields():
    """Grid, threads, LDS and slab bytes of three plans: the 256x160 tile, a split 64x128 tile with an adapter, a batched K-grouped launch."""
    pl = plan(block(1024, 10240, 1280))
    assert (pl.tile, pl.mode, pl.r16, pl.stages, pl.kg, pl.bt, pl.epi, pl.ln, pl.splitk) == (7, 0, 0, 3, 0, 0, 0, 0, 1)
    assert (pl.grid_x, pl.grid_y, pl.threads, pl.lds_bytes, pl.slab_bytes) == (256, 1, 512, 159744, 163840)
    assert pl.stages_req == 4 and plan(block(1024, 10240, 1280, stages=2)).stages_req == 2      # (asked for "as deep as fits": three stages of 256x160 fit; asked for two)
    pl = plan(block(256, 1280, 5120, rank=16))
    assert (pl.tile, pl.mode, pl.r16, pl.stages, pl.kg, pl.bt, pl.epi, pl.ln, pl.splitk) == (2, 0, 1, 4, 0, 0, 0, 0, 4)
    assert (pl.grid_x, pl.grid_y, pl.threads, pl.lds_bytes, pl.slab_bytes) == (160, 1, 512, 109056, 40960)
    pl = plan(block(154, 2048, 2560, rank=32, lora_group_k=1280, batch=BASE + 0x3000, n_batch=70))
    assert (pl.tile, pl.mode, pl.r16, pl.stages, pl.kg, pl.bt, pl.epi, pl.ln, pl.splitk) == (2, 0, 2, 4, 4, 1, 0, 0, 1)
    assert (pl.grid_x, pl.grid_y, pl.threads, pl.lds_bytes, pl.slab_bytes) == (48, 70, 512, 131584, 49152)


# ---------------------------------------------------------------------------------------------- 3. refusals: those of the launch entry, same code, same text
# Every refusal that tests/test_gemm_exact_gpu.py and tests/test_conv_exact_gpu.py assert on the device, as the same cross products over the same lists and with
# the same message substrings (the lists are restated here: importing a GPU test file would need its fixtures).  `conv`: the convolution file's mode 1 cases.
REJECTED = [(7, 32, "tile id"), (7, 64, "tile id"), (8, 32, "tile id"), (8, 64, "tile id"), (6, 64, "does not fit the 160 KB LDS")]      # both files' REJECTED
GROUP_N_REJECTED = [(1, 64), (2, 64), (8, 64), (8, 128), (4, 64), (6, 128), (7, 128)]                                                    # test_group_n_rejected
BATCH = dict(batch=BASE + 0x3000, n_batch=3)
GPU_REFUSED = (
    # test_rejected of either file: (tile, rank pad) without a kernel, under both ring requests
    [(f"{'conv' if conv else 'product'}, tile {t}, rank pad {pad}, stages {st}", block(256 if conv else 105, 200, 576 if conv else 192, conv=conv, rank=pad, tile=t, stages=st, splitk=1),
      ERR_UNSUPPORTED, why) for conv in (False, True) for t, pad, why in REJECTED for st in (0, 2)] +
    # test_rejected_tile_id, test_planner_keeps_the_forced_tile
    [("product, tile id 9", block(105, 200, 192, tile=9, splitk=1), ERR_UNSUPPORTED, "tile id"),
     ("product, tile id 9, adapter", block(105, 200, 192, rank=16, tile=9, splitk=1), ERR_UNSUPPORTED, "tile id"),
     ("conv, tile id 9", block(105, 200, 576, conv=True, tile=9, splitk=1), ERR_UNSUPPORTED, "tile id")] +
    # test_group_n_rejected, test_second_segment_grouped_rejected
    [(f"lora_group_n {w} on tile {t}", block(105, 2 * w, 192, rank=16, tile=t, splitk=1, lora_group_n=w), ERR_SHAPE, f"lora_group_n={w} is not a multiple") for t, w in GROUP_N_REJECTED] +
    [(f"x2_group_n 64 on tile {t}", block(105, 128, 192, tile=t, splitk=1, **seg2(x2_group_n=64)), ERR_SHAPE, "x2_group_n=64 is not a multiple") for t in (1, 2, 4, 5, 6, 7, 8)] +
    # test_group_k_rejected
    [(f"lora_group_k on tile {t}", block(105, 200, 128, rank=16, tile=t, splitk=1, lora_group_k=64), ERR_UNSUPPORTED, "lora_group_k needs mode 0 and tile 1..3") for t in (4, 5, 6, 7, 8)] +
    # test_batched_rejected: plain, adapter groups, K groups on tile 4
    [("batched on tile 4", block(105, 200, 192, tile=4, splitk=1, **BATCH), ERR_UNSUPPORTED, "tile 1..3"),
     ("batched on tile 4, adapter groups", block(105, 256, 192, rank=16, tile=4, splitk=1, lora_group_n=128, **BATCH), ERR_UNSUPPORTED, "tile 1..3"),
     ("batched on tile 4, K groups", block(105, 200, 128, rank=16, tile=4, splitk=1, lora_group_k=64, **BATCH), ERR_UNSUPPORTED, "tile 1..3")])
REFUSED = GPU_REFUSED + [
    ("256x256 with rank pad 64: the whole text", block(105, 200, 192, rank=64, tile=6), ERR_UNSUPPORTED, "tile 256x256 with LoRA rank pad 64 does not fit the 160 KB LDS"),
    ("64-wide adapter groups on a 128-column tile", block(105, 128, 192, rank=16, tile=1, lora_group_n=64), ERR_SHAPE, "lora_group_n=64 is not a multiple of the 128-column tile"),
    ("64-wide adapter groups on a 160-column tile", block(105, 128, 192, rank=16, tile=8, lora_group_n=64), ERR_SHAPE, "lora_group_n=64 is not a multiple of the 160-column tile"),
    ("128-wide adapter groups on a 160-column tile", block(105, 256, 192, rank=16, tile=8, lora_group_n=128), ERR_SHAPE, "lora_group_n=128 is not a multiple"),
    ("128-wide adapter groups on a 256-column tile", block(105, 256, 192, rank=16, tile=6, lora_group_n=128), ERR_SHAPE, "lora_group_n=128 is not a multiple of the 256-column tile"),
    ("96-wide adapter groups, no tile takes them", block(105, 192, 192, rank=16, lora_group_n=96), ERR_SHAPE, "lora_group_n=96 is not a multiple"),
    ("64-wide second-segment groups on a 128-column tile", block(105, 128, 192, tile=2, **seg2(x2_group_n=64)), ERR_SHAPE, "x2_group_n=64 is not a multiple of the 128-column tile"),
    ("64-wide second-segment groups on a 160-column tile", block(105, 128, 192, tile=7, **seg2(x2_group_n=64)), ERR_SHAPE, "x2_group_n=64 is not a multiple of the 160-column tile"),
    ("K groups on a forced tile above 3", block(105, 200, 128, rank=16, tile=4, lora_group_k=64), ERR_UNSUPPORTED, "lora_group_k needs mode 0 and tile 1..3 (tile 4)"),
    ("K groups on a 160-column tile", block(105, 200, 128, rank=16, tile=8, lora_group_k=64), ERR_UNSUPPORTED, "lora_group_k needs mode 0 and tile 1..3 (tile 8)"),
    ("batched on a forced tile above 3", block(105, 200, 192, tile=4, batch=BASE + 0x3000, n_batch=3), ERR_UNSUPPORTED, "batched launch needs mode 0 and tile 1..3 (tile 4)"),
    ("batched convolution", block(64, 200, 576, conv=True, tile=1, batch=BASE + 0x3000, n_batch=3), ERR_UNSUPPORTED, "batched launch needs mode 0 and tile 1..3 (tile 1)"),
    ("n_batch 0", block(105, 200, 192, batch=BASE + 0x3000, n_batch=0), ERR_SHAPE, "n_batch=0"),
    ("n_batch 65536", block(105, 200, 192, batch=BASE + 0x3000, n_batch=65536), ERR_SHAPE, "n_batch=65536"),
    ("folded LayerNorm without adapter or GEGLU", block(256, 1280, 1280, **ln()), ERR_UNSUPPORTED, "folded LayerNorm exists for rank-16 adapter products and for ff.net.0.proj + GEGLU (lora_R 0, epi_op 0, tile 2)"),
    ("folded LayerNorm + GEGLU on tile id 9", block(256, 1280, 1280, tile=9, **ln(), **epi(1)), ERR_UNSUPPORTED, "epi_op 1, tile 9)"),
    ("fused epilogue on tile id 9", block(256, 1280, 1280, tile=9, **epi(3)), ERR_UNSUPPORTED, "fused epilogue 3 needs mode 0 without LoRA (tile 9)"),
    ("split without a workspace", block(105, 200, 576, ws=False, tile=1, splitk=3), ERR_SHAPE, "split-K workspace too small (2 tiles x 3 splits x 65536 B)"),
    ("split with too few counters", block(105, 200, 576, tile=1, splitk=3, ws_cnt_len=1), ERR_SHAPE, "split-K workspace too small"),
    ("split with too small a slab", block(105, 200, 576, tile=1, splitk=3, ws_slab_bytes=6 * 65536 - 1), ERR_SHAPE, "split-K workspace too small"),
    ("misaligned operand", block(105, 200, 192, X=BASE + 8), ERR_ALIGN, "operand base pointers must be 16-byte aligned"),
    ("K no multiple of 64", block(105, 200, 200), ERR_SHAPE, "K=200 K2=0 must be positive multiples of 64"),
]


@pytest.mark.parametrize("what,p,code,text", REFUSED, ids=[c[0] for c in REFUSED])
def test_refusals_are_those_of_the_launch_entry(what, p, code, text):
    rc, msg = refusal(p)
    assert rc == code and text in msg and msg.startswith("sdlt_gemm_bf16: "), msg


def test_a_refused_route_leaves_the_plan_alone():
    pl = _lib.GemmPlan(tile=-7)
    assert _lib.load().sdlt_gemm_route(ctypes.byref(block(105, 200, 192, tile=9)), ctypes.byref(pl)) == ERR_UNSUPPORTED and pl.tile == -7
    assert ctypes.sizeof(_lib.GemmPlan) == 64
