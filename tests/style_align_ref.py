"""Style-aligned batches in fp64 torch: the two formulas of include/sdlt_kernels.h (sdlt_adain_affine, sdlt_attn_shared_fwd), nothing else."""
import torch


def reference_row(b, G, gs=1):
    return (b // (G * gs)) * (G * gs) + b % gs


def adain_affine(X, *, B, N, G, gs=1, dtype=torch.float64):
    """X [B N, C2] -> A, S [B, C2]: A = std_r / std_b, S = mean_r - A mean_b, unbiased variance, std = sqrt(var + 1e-5); exactly (1, 0) for a reference."""
    x = X.to(dtype).view(B, N, -1)
    mean, std = x.mean(1), (x.var(1, unbiased=True) + 1e-5).sqrt()
    r = [reference_row(b, G, gs) for b in range(B)]
    A = std[r] / std
    S = mean[r] - A * mean
    own = torch.tensor([b == rb for b, rb in enumerate(r)])
    A[own], S[own] = 1.0, 0.0
    return A, S


def attn_shared(Q, K, V, *, B, H, N, d, G, scale, shift, tables=None, gs=1, round_qk=None, dtype=torch.float64):
    """Q, K, V [B N, >= H d] -> O [B N, H d] in `dtype`.  tables = (Aq, Sq, Ak, Sk) [B, H d] or None.  round_qk: a function applied to q' and k' (the
    emulation's bf16 rounding); None: exact."""
    C = H * d
    q, k, v = (t[:, :C].to(dtype).view(B, N, H, d).transpose(1, 2) for t in (Q, K, V))      # [B, H, N, d]
    qa, ka = q, k
    if tables is not None:
        Aq, Sq, Ak, Sk = (t[:, :C].to(dtype).reshape(B, H, 1, d) for t in tables)
        qa, ka = Aq * q + Sq, Ak * k + Sk
    if round_qk is not None:
        qa, ka = round_qk(qa), round_qk(ka)
    out = torch.empty(B, H, N, d, dtype=dtype)
    for b in range(B):
        r = reference_row(b, G, gs)
        s, vv = scale * qa[b] @ ka[b].transpose(1, 2), v[b]
        if r != b:
            s = torch.cat([s, scale * qa[b] @ k[r].transpose(1, 2) + shift], 2)
            vv = torch.cat([vv, v[r]], 1)
        out[b] = torch.softmax(s, 2) @ vv
    return out.transpose(1, 2).reshape(B * N, C)
