"""Exact-arithmetic reference of multi-head softmax attention, forward and backward (sdlt_attn_fwd / sdlt_attn_bwd, sdlt_attn_splitsum_batch), with
operands that make a softmax exact.  Plain torch in fp64 on the CPU; imports nothing from the project.

The contract restated (include/sdlt_kernels.h, ops.attn_fwd / attn_bwd, and tests/emu_ops.py, whose attn_fwd / attn_bwd are its executable form):

  S = scale * Q K^T per (batch, head), keys >= Nk and (causal) keys > query masked;  P = softmax(S);  O = P V;  L = logsumexp(S)  [B, H, Nq] fp32
  D = rowsum(dO o O);  dS = P o (dO V^T - D);  dQ = scale dS K;  dK = scale dS^T Q;  dV = P^T dO          (query rows >= Nq take no part)
  * Q, O, dO, dQ are [B * Nqp, ld] views, K, V, dK, dV [B * Nkp, ld] views, head h in columns [h d, (h + 1) d); Nqp, Nkp multiples of 8.
  * pad rows of dK and dV (keys Nk .. Nkp of every batch element) receive ZEROS (emu_ops.attn_bwd: a masked key has P = 0, so its gradient is 0);
    with accumulate_dk the pad rows of dK keep what they held (previous + 0), dV is always overwritten.
  * pad rows of O and dQ (queries Nq .. Nqp) are written with finite values that no caller reads (the kernels write an average of V, and zeros);
    the tests mask exactly those rows and require them finite.
  * accumulate_dq / accumulate_dk (cross routes): dQ, dK = bf16(previous + result), one rounding.
  * qsplit > 1: dK32 / dV32 are [qsplit][B * Nkp][ld32] fp32 slabs whose sum over the split index is dK (scaled) / dV.  Rows of pad keys are zeros on
    the BWD_SPLIT route and left untouched on the cross routes; the slab sum writes zeros to the pad rows of dK / dV without reading them.
  * what a kernel may LOAD: K / V rows up to Nkp (whole tiles; scores masked past Nk), Q / dO / O rows up to Nqp in the backward (key-major tiles);
    never a row past Nkp / Nqp, never a column outside the heads.  So pad rows hold finite bait here and everything else around an operand NaN.

Why these operands are exact.  Per head the first `ncode` columns are a signed one-hot class code of magnitude 32: query i of class c has +-32 in
column c // 2 (sign by c % 2), and so has every key of class c; all other code columns of a key hold -1 / 0 / 1.  The remaining columns come in
pairs: Q carries (x, x), K carries (y, -y), x, y in -2 .. 2, which cancel in every score.  With scale = 0.125 (every head width) a query scores 128
on the t keys of its class, -128 on the class of the other sign, -4 / 0 / 4 on everything else: the winners tie exactly and every loser lies
>= 124 * log2(e) = 178.9 octaves below, past the fp32 underflow.  Class sizes cycle 1, 2, 4, 8, so P = 1 / t or 0, O = sum(V) / t, and
dS = (t dP_j - sum_winners dP) / t^2 with |numerator| < 256 are bf16 numbers, every product an fp32 sum of multiples of 2^-9 below 2^15:
no result depends on tile, split, wave group or summation order (tests/test_attn_exact_cpu.py asserts all of it for every case below).
"""
import functools

import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SCALE = 0.125                      # for every head width: the multiplication is exact
LOG2E = 1.4426950408889634
CODE, BAIT = 32.0, 64.0            # class code magnitude; the code a pad key carries (it would score 256: beat every winner)
V_PAD, Q_PAD_DO, O_PAD = 96.0, 2.0, 5.0
SIZES = (1, 2, 4, 8)
PRE, SLACK = 2, 64                 # rows in front of an operand / behind an output inside its buffer
NPATTERN = 3                       # distinct class layouts per case; head (b, h) uses pattern (b * H + h) % 3


def R(name, dp=64, ks=1, dv48=False, five=False, prep=False, splitsum=False):
    return dict(route=name, dp=dp, ks=ks, dv48=dv48, five=five, prep=prep, splitsum=splitsum)


def _case(name, B, H, Nq, Nk, Nkp, d, fwd, bwd, causal=False, qsplit=1, ocol=8):
    return dict(name=name, B=B, H=H, Nq=Nq, Nk=Nk, Nkp=Nkp, Nqp=(Nq + 7) // 8 * 8, d=d, causal=causal, qsplit=qsplit, ocol=ocol, fwd=fwd, bwd=bwd)


# ocol: column (bf16 elements) at which the output views O / dQ start inside their buffers: 8 = 16-byte aligned, 4 = misaligned by 8 bytes
CASES = [
    _case("self32_ks2", 2, 2, 256, 256, 256, 64, R("FWD32", ks=2), R("BWD_BOTH32", ks=2, prep=True)),
    _case("self32_ks1", 1, 2, 192, 64, 64, 64, R("FWD32"), R("BWD_BOTH32", prep=True)),
    _case("self32_misaligned", 2, 2, 256, 256, 256, 64, R("FWD16_KS2", ks=2), R("BWD_BOTH16", prep=True), ocol=4),
    _case("ks2_d40", 1, 8, 250, 257, 264, 40, R("FWD16_KS2", ks=2), R("BWD_BOTH16", prep=True)),
    _case("self16_more_keys", 1, 3, 100, 193, 200, 64, R("FWD16"), R("BWD_BOTH16", prep=True)),
    _case("dp96", 1, 2, 100, 129, 136, 80, R("FWD16", dp=96), R("BWD_BOTH16", dp=96, prep=True)),
    _case("dp160", 1, 2, 130, 130, 136, 160, R("FWD16", dp=160), R("BWD_BOTH16", dp=160, prep=True)),
    _case("cross_five_80", 1, 2, 200, 77, 80, 64, R("FWD16"), R("BWD_CROSS_ROLES", five=True, splitsum=True), qsplit=2),
    _case("cross_five_128", 2, 3, 300, 77, 128, 64, R("FWD16"), R("BWD_CROSS_ROLES", five=True, splitsum=True), qsplit=4),
    _case("cross_64_keys", 1, 2, 136, 64, 64, 64, R("FWD16"), R("BWD_CROSS_ROLES", splitsum=True), qsplit=3),
    _case("cross_dv48", 1, 2, 68, 40, 40, 40, R("FWD16", dv48=True), R("BWD_CROSS_ROLES", splitsum=True), qsplit=2),
    _case("cross_dp96", 2, 3, 200, 77, 128, 80, R("FWD16", dp=96), R("BWD_CROSS", dp=96, five=True, splitsum=True), qsplit=3),
    _case("split_slabs", 2, 2, 316, 77, 128, 160, R("FWD16", dp=160), R("BWD_SPLIT", dp=160, splitsum=True), qsplit=4),
    _case("split_grid_d64", 1, 683, 128, 64, 64, 64, R("FWD32"), R("BWD_SPLIT")),
    _case("split_grid_d40", 5, 205, 60, 64, 64, 40, R("FWD16", dv48=True), R("BWD_SPLIT", dv48=True)),
    _case("causal", 2, 2, 77, 77, 80, 64, R("FWD16"), R("BWD_BOTH16", prep=True), causal=True),
    # pad keys behind whole key tiles: the 32-row backward stores no pad rows, so the planner keeps the backward on the 16-row kernel (dK / dV pad rows: zeros)
    _case("self32_pad_keys", 1, 2, 192, 64, 72, 64, R("FWD32"), R("BWD_BOTH16", prep=True)),
]
BY_NAME = {c["name"]: c for c in CASES}
CROSS = tuple(c["name"] for c in CASES if c["bwd"]["route"] in ("BWD_CROSS_ROLES", "BWD_CROSS"))
SELF = tuple(c["name"] for c in CASES if c["bwd"]["route"] in ("BWD_BOTH32", "BWD_BOTH16"))      # the routes with a D pre-pass (d_ready)


def rounded(acc, dtype):
    """The fp64 result in the output's format.  The honest softmax leaves 2^-178 on the losers instead of 0, so `acc` is an fp32 number up to that
    dust (asserted: nothing above 2^-140 is lost); then one RNE rounding for bf16."""
    f = acc.to(F32)
    assert float((f.to(F64) - acc).abs().max()) < 2.0 ** -140, "the operands do not keep the result exact in fp32"
    return f if dtype == F32 else f.to(dtype)


# ---------------------------------------------------------------------------------------------------------------- operands
def _n_classes(Nk, d):
    """A multiple of 4 (each size equally often, two classes per code column, an even number of pair columns left), on <= 60 % of the keys and <= 3 d / 8 columns."""
    n, used = 0, 0
    while used + SIZES[n % 4] <= 0.6 * Nk and (n + 1) <= 2 * (3 * d // 8):
        used += SIZES[n % 4]
        n += 1
    return max(4, n // 4 * 4)


def _place(g, Nk, n, causal):
    """Keys of each class.  The first classes are placed on purpose: only in the last key tile (0: the last key, 6: four keys), only in the first
    (1, 4: key 0), one per quarter (2), one per eighth - both wave groups of a key-split kernel (3), first and last tile (5); the rest at random
    (causal: at random in the front four fifths, so that a later query sees the whole class)."""
    free = [True] * Nk
    members = []

    def take(pos):
        pos %= Nk
        while not free[pos]:
            pos = (pos + 1) % Nk
        free[pos] = False
        return pos

    want = {0: [Nk - 1], 1: [3, 17], 2: [q * Nk // 4 + 5 for q in range(4)], 3: [e * Nk // 8 + 2 for e in range(8)], 4: [0], 5: [7, Nk - 2],
            6: [Nk - 3 - e for e in range(4)]}
    for c in (4, 0, 6, 5, 1, 2, 3):
        if c < n:
            want[c] = [take(p) for p in want[c]]
    for c in range(n):
        if c in want:
            members.append(sorted(want[c]))
            continue
        pool = [k for k in range(Nk * 4 // 5 if causal else Nk) if free[k]]
        pick = torch.randperm(len(pool), generator=g)[:SIZES[c % 4]].tolist()
        members.append(sorted(take(pool[i]) for i in pick))
    return members


def _query_classes(g, Nq, n, members, causal):
    if not causal:      # every class equally often, in random order
        return torch.cat([torch.randperm(n, generator=g) for _ in range(-(-Nq // n))])[:Nq].tolist()
    # causal: query i may take a class of which it sees 1, 2, 4 or 8 keys.  From the last query down, first give every class one query that sees all
    # of it (latest last key first: the only order in which all find one), then whatever tie count this head has used least.
    out, whole, used = [0] * Nq, set(), {t: 0 for t in SIZES}
    for i in reversed(range(Nq)):
        seen = {c: sum(k <= i for k in members[c]) for c in range(n)}
        ok = [c for c in range(n) if seen[c] in SIZES]
        full = [c for c in ok if seen[c] == len(members[c]) and c not in whole]
        c = max(full, key=lambda c: members[c][-1]) if full else min(ok, key=lambda c: (used[seen[c]], c))
        if full:
            whole.add(c)
        used[seen[c]] += 1
        out[i] = c
    return out


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


@functools.lru_cache(maxsize=None)
def operands(name):
    """CPU bf16 operands of a case, pad rows included: Q, dO [B * Nqp, C], K, V [B * Nkp, C]; dQ0 / dK0: what the accumulating launches find;
    `classes`: per pattern (members, class of each query)."""
    c = BY_NAME[name]
    B, H, Nq, Nk, Nkp, Nqp, d = c["B"], c["H"], c["Nq"], c["Nk"], c["Nkp"], c["Nqp"], c["d"]
    g = torch.Generator().manual_seed(1000 + 7 * CASES.index(c))
    n = _n_classes(Nk, d)
    ncode = n // 2
    npair = (d - ncode) // 2
    nv, vmax = (3, 3) if d <= 80 else (4, 2)          # |dP| <= nv * vmax * 2 <= 18: the numerator of dS stays below 256
    Q, K = torch.zeros(B, H, Nqp, d, dtype=F64), torch.zeros(B, H, Nkp, d, dtype=F64)
    V = torch.zeros(B, H, Nkp, d, dtype=F64)
    dO = _ints(g, -2, 2, B, H, Nqp, d)
    dO[:, :, Nq:] = Q_PAD_DO
    heads = torch.arange(B * H).view(B, H)
    classes = []
    for pat in range(NPATTERN):
        members = _place(g, Nk, n, c["causal"])
        qcls = _query_classes(g, Nq, n, members, c["causal"])
        classes.append((members, qcls))
        sel = (heads % NPATTERN == pat)
        nh = int(sel.sum())
        if nh == 0:
            continue
        q, k, v = torch.zeros(nh, Nqp, d, dtype=F64), torch.zeros(nh, Nkp, d, dtype=F64), torch.zeros(nh, Nkp, d, dtype=F64)
        # queries: the class code, pad rows too (bait: a pad query that is not masked adds to dK / dV), and the (x, x) pairs
        qc = torch.tensor(qcls + [r % n for r in range(Nqp - Nq)])
        q[:, torch.arange(Nqp), qc // 2] = CODE * (1 - 2 * (qc % 2)).to(F64)
        x = _ints(g, -2, 2, nh, Nqp, npair)
        q[:, :, ncode:] = torch.stack([x, x], -1).reshape(nh, Nqp, 2 * npair)
        # keys: -1 / 0 / 1 in the code columns (at random; the r-th key of a class (r + column) % 3 - 1, so that the keys of a class differ in every
        # column and dQ picks the column up), the own column of a class key +-32; the (y, -y) pairs
        k[:, :Nk, :ncode] = _ints(g, -1, 1, nh, Nk, ncode)
        for cl, mem in enumerate(members):
            k[:, mem, :ncode] = ((torch.arange(len(mem))[:, None] + torch.arange(ncode)[None, :]) % 3 - 1).to(F64)
            k[:, mem, cl // 2] = CODE * (1 - 2 * (cl % 2))
        y = _ints(g, -2, 2, nh, Nk, npair)
        k[:, :Nk, ncode:] = torch.stack([y, -y], -1).reshape(nh, Nk, 2 * npair)
        for r in range(Nk, Nkp):      # pad keys: a code that beats the winners of one class (both signs in turn)
            k[:, r, (r // 2) % ncode] = BAIT * (1 - 2 * (r % 2))
        # values: nv entries per key, walking a column permutation in key order (class keys first), so that the class keys cover every column
        order = sorted(range(Nk), key=lambda j: (not any(j in m for m in members), j))
        perm = torch.randperm(d, generator=g)
        cols = torch.empty(Nk, nv, dtype=torch.long)
        cols[order] = perm[(torch.arange(Nk)[:, None] * nv + torch.arange(nv)[None, :]) % d]
        sign = (1 - 2 * _ints(g, 0, 1, d))[cols]          # one sign per column: the values of a class never cancel in O
        v[:, :Nk].scatter_(2, cols[None].expand(nh, Nk, nv), _ints(g, 1, vmax, nh, Nk, nv) * sign[None])
        v[:, Nk:] = V_PAD
        # dK's code column c // 2 is 4 sum_i dS_ij over the queries of class c: of the two classes of a column the odd one has 2 or 8 keys; where chance
        # makes that sum zero for all its keys, move one dO entry of the class's last query by one (placing operands, not computing results)
        do = dO[sel]
        for cl in range(1, n, 2):
            mem, I = members[cl], [i for i in range(Nq) if qcls[i] == cl]
            vis = torch.tensor([[(not c["causal"]) or j <= i for j in mem] for i in I]).to(F64)          # [queries, keys]
            dP = do[:, I] @ v[:, mem].transpose(-1, -2) * vis
            t = vis.sum(-1, keepdim=True)
            dead = ((vis * (dP - dP.sum(-1, keepdim=True) / t) / t).sum(1) == 0).all(-1)
            others = set(cols[mem[1:]].flatten().tolist())
            col = next((x for x in cols[mem[0]].tolist() if x not in others), int(cols[mem[0], 0]))          # a column in which only the class's first key has a value
            old = do[dead, I[-1], col]
            do[dead, I[-1], col] = torch.where(old < 2, old + 1, old - 1)
        dO[sel] = do
        Q[sel], K[sel], V[sel] = q, k, v

    def flat(t, Np):
        return t.permute(0, 2, 1, 3).reshape(B * Np, H * d).to(BF)
    out = dict(Q=flat(Q, Nqp), K=flat(K, Nkp), V=flat(V, Nkp), dO=flat(dO, Nqp), classes=classes, n_classes=n, ncode=ncode)
    out["dQ0"] = _ints(g, -3, 3, B * Nqp, H * d).to(BF)
    out["dK0"] = _ints(g, -3, 3, B * Nkp, H * d).to(BF)
    return out


# ---------------------------------------------------------------------------------------------------------------- the reference
def _heads(t, B, Np, H, d):
    return t.to(F64).reshape(B, Np, H, d).permute(0, 2, 1, 3)


def _flat(t):
    B, H, Np, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * Np, H * d)


@functools.lru_cache(maxsize=None)
def reference(name):
    """fp64 results of a case before the output rounding, computed once and never modified: P, S (scaled scores, masked = -inf), O, L, D, dS, dQ, dK, dV
    in the operands' layouts ([B * Np, C]; P, S, dS [B, H, Nq, Nk]; L, D [B * H * Nq]).  An ordinary masked softmax and its gradient - no use of the ties."""
    c = BY_NAME[name]
    B, H, Nq, Nk, Nkp, Nqp, d = c["B"], c["H"], c["Nq"], c["Nk"], c["Nkp"], c["Nqp"], c["d"]
    op = operands(name)
    q, k, v, do = _heads(op["Q"], B, Nqp, H, d)[:, :, :Nq], _heads(op["K"], B, Nkp, H, d)[:, :, :Nk], _heads(op["V"], B, Nkp, H, d)[:, :, :Nk], \
        _heads(op["dO"], B, Nqp, H, d)[:, :, :Nq]
    s = (q @ k.transpose(-1, -2)) * SCALE
    if c["causal"]:
        s = s.masked_fill(torch.triu(torch.ones(Nq, Nk, dtype=torch.bool), diagonal=1), float("-inf"))
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    z = e.sum(-1, keepdim=True)
    P = e / z
    L = (m + torch.log(z)).squeeze(-1)
    O = P @ v
    D = (do * O).sum(-1, keepdim=True)
    dS = P * (do @ v.transpose(-1, -2) - D)
    dQ, dK, dV = SCALE * (dS @ k), SCALE * (dS.transpose(-1, -2) @ q), P.transpose(-1, -2) @ do

    def padded(t, Np):
        full = torch.zeros(B, H, Np, d, dtype=F64)
        full[:, :, :t.shape[2]] = t
        return _flat(full)
    return dict(P=P, S=s, dS=dS, O=padded(O, Nqp), dQ=padded(dQ, Nqp), dK=padded(dK, Nkp), dV=padded(dV, Nkp), L=L.reshape(-1), D=D.reshape(-1))


def row_mask(c, Np, N):
    """[B * Np, 1] bool: the logical rows (n < N of every batch element)."""
    return (torch.arange(c["B"] * Np) % Np < N)[:, None]


def l_bound(L_ref):
    """|L - L_ref| allowed: scale * LOG2E, tmax * sl2, log2f, the add and the divide by LOG2E - five roundings / approximations of at most about one fp32
    ulp of |L log2e| each; 8 ulp of max(|L_ref|, 1)."""
    return 8 * 2.0 ** -23 * L_ref.abs().clamp(min=1.0)


# ---------------------------------------------------------------------------------------------------------------- frames
def frames(name):
    """Where every tensor of a launch lives: name -> (buffer, first row, first column, rows, columns); buffers: name -> (rows, width, dtype).
    Q | K | V are column slices of one [rows, 3 C + 16] buffer when queries and keys have the same padded count, else Q of its own buffer of that width and
    K | V of another; dQ | dK | dV likewise (starting at column `ocol`); O and dO are slices of [rows, C + 24] buffers; the fp32 slabs of [rows, C + 8] ones;
    L and D sit 4 floats into 1-D buffers.  Inputs have PRE rows in front and behind, outputs PRE in front and SLACK behind."""
    c = BY_NAME[name]
    B, H, Nkp, Nqp, d, oc = c["B"], c["H"], c["Nkp"], c["Nqp"], c["d"], c["ocol"]
    C = H * d
    W = 3 * C + 16
    rq, rk = B * Nqp, B * Nkp
    one = Nqp == Nkp
    bufs, t = {}, {}
    for pre, tail, off, names in (("in", PRE, 8, ("Q", "K", "V")), ("out", SLACK, oc, ("dQ", "dK", "dV"))):
        if one:
            bufs[pre + "_qkv"] = (PRE + rq + tail, W, BF)
            for i, nm in enumerate(names):
                t[nm] = (pre + "_qkv", PRE, off + i * C, rq, C)
        else:
            bufs[pre + "_q"], bufs[pre + "_kv"] = (PRE + rq + tail, W, BF), (PRE + rk + tail, W, BF)
            t[names[0]] = (pre + "_q", PRE, off, rq, C)
            t[names[1]], t[names[2]] = (pre + "_kv", PRE, off + C, rk, C), (pre + "_kv", PRE, off + 2 * C, rk, C)
    bufs["in_o"], bufs["in_do"], bufs["out_o"] = (PRE + rq + PRE, C + 24, BF), (PRE + rq + PRE, C + 24, BF), (PRE + rq + SLACK, C + 24, BF)
    t["O_in"], t["dO"], t["O"] = ("in_o", PRE, 8, rq, C), ("in_do", PRE, 16, rq, C), ("out_o", PRE, oc, rq, C)
    if c["qsplit"] > 1:
        for nm in ("dK32", "dV32"):
            bufs["out_" + nm] = (PRE + c["qsplit"] * rk + SLACK, C + 8, F32)
            t[nm] = ("out_" + nm, PRE, 4, c["qsplit"] * rk, C)
    for nm in ("L", "D"):
        bufs["out_" + nm] = (1, 4 + B * H * c["Nq"] + SLACK, F32)
        t[nm] = ("out_" + nm, 0, 4, 1, B * H * c["Nq"])
    return bufs, t


def address(name, tensor, base=0):
    """(byte offset of a tensor's first element inside its buffer + base, leading dimension in elements)."""
    bufs, t = frames(name)
    buf, r0, c0, _, _ = t[tensor]
    _, width, dtype = bufs[buf]
    return base + (r0 * width + c0) * (2 if dtype == BF else 4), width



def fill_block(p, name, ptr, backward, *, d_ready=False, defer_splitsum=False, accumulate=False, zero_D=False):
    """Fill an sdlt_attn_params mirror `p` for a case the way ops.attn_fwd / ops.attn_bwd do; ptr(tensor) -> address of its first element.  The leading
    dimensions are those of frames(): the CPU file (made-up 256-byte-aligned buffer addresses) and the GPU file (real ones) build the same block."""
    c = BY_NAME[name]
    ld = lambda nm: address(name, nm)[1]      # noqa: E731
    p.Q, p.ldq, p.K, p.ldk, p.V, p.ldv = ptr("Q"), ld("Q"), ptr("K"), ld("K"), ptr("V"), ld("V")
    p.B, p.H, p.Nq, p.Nk, p.Nqp, p.Nkp, p.d = c["B"], c["H"], c["Nq"], c["Nk"], c["Nqp"], c["Nkp"], c["d"]
    p.scale, p.qsplit, p.causal = SCALE, 1, int(c["causal"])
    if not backward:
        p.O, p.ldo, p.L = ptr("O"), ld("O"), ptr("L")
        if zero_D:
            p.D = ptr("D")
        return p
    p.defer_splitsum, p.d_ready = int(defer_splitsum), int(d_ready)
    p.O, p.ldo, p.L, p.dO, p.lddo, p.D = ptr("O_in"), ld("O_in"), ptr("L"), ptr("dO"), ld("dO"), ptr("D")
    p.dQ, p.lddq, p.dK, p.lddk, p.dV, p.lddv = ptr("dQ"), ld("dQ"), ptr("dK"), ld("dK"), ptr("dV"), ld("dV")
    p.qsplit = c["qsplit"]
    p.accumulate_dq = p.accumulate_dk = int(accumulate)
    if c["qsplit"] > 1:
        p.dK32, p.dV32, p.ld32 = ptr("dK32"), ptr("dV32"), ld("dK32")
    return p
