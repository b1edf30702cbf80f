"""What the attention tests share: a float64 chunk-attention reference that also returns the
softmax-weighted mean of |V|, the per-element error bound built on it, and the exact map of a tail
with zero keys and one-hot values.

The bound.  extend.hip rounds each softmax weight pᵢ (relative to the running maximum, so pᵢ ≤ 2⁸) to
the K/V dtype before the weights·V product on the matrix core; the row sum stays fp32 from the
unrounded weights.  Rounding changes pᵢ by at most u·pᵢ, u = 2⁻¹¹ (float16) or 2⁻⁸ (bfloat16), so
output element d of a query moves by at most

    Σᵢ u·pᵢ·|vᵢd| / Σᵢ pᵢ = u·A_d,      A = softmax(q·Xᵀ·scale)·|Y|,

u times the softmax-weighted mean of |V| in that channel — not u·max|V|.  With the decode family's
rtol = 2e-4 and atol = 2e-5·vmax (fp32 summation order, hardware exp2; tests/test_gpu_decode.py) the
elementwise check is

    |out − ref| ≤ 2e-4·|ref| + 2e-5·vmax + 2u·A,      vmax = max(max|V'|, max|tail V|, 1).

The factor 2 on u covers float16 underflow of very small weights and the lazily trailing maximum.
A ≤ vmax everywhere, so this is never looser than (2e-5 + 2u)·vmax; float32 (u = 0) is the decode
tests' tolerance unchanged.  tests/test_attn_bound_host.py shows on the CPU that a correct kernel with
rounded weights stays far inside the bound and that off-by-one kernels do not."""
from collections import namedtuple

import torch

U = {"float16": 2.0 ** -11, "bfloat16": 2.0 ** -8, "float32": 0.0}
RTOL, ATOL = 2e-4, 2e-5

Ref = namedtuple("Ref", "out A")   # float64 [.., D] each
TD = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}

# The ground-truth cases of tests/test_gpu_extend.py (and, without the bits, of tests/test_attn_bound_host.py).
SHAPES = [
    # S, Hkv, D, Hq
    (700, 4, 128, 4),        # G = 1
    (900, 8, 128, 8),        # F = 1024
    (620, 4, 128, 8),        # G = 2
    (1000, 4, 128, 16),      # G = 4
]
# (T, older tail rows): T = 1, 2 the smallest steps; 5 below one 16-query MFMA group, 16 exactly one, 17 one
# past; 70 past a pass of query rows.  Older rows: none, a few, past one 64-row round, several tail splits.
STEPS = [
    ((1, 0), (2, 3), (5, 257), (16, 1500), (17, 0), (70, 3)),
    ((1, 1500), (2, 257), (5, 3), (16, 0), (17, 257), (70, 1500)),
    ((1, 3), (2, 0), (5, 1500), (16, 257), (17, 3), (70, 0)),
    ((1, 257), (2, 1500), (5, 0), (16, 3), (17, 1500), (70, 257)),
]


def visible(T, n, device=None):
    """vis(t) = max(0, n − (T − 1 − t)) for t < T: the tail rows query t of a T-token chunk sees."""
    return (int(n) - (T - 1 - torch.arange(T, device=device))).clamp(min=0)


# The queries of the ground-truth cases.  With N(0, 1) queries and keys a single row among N carries a weight
# of about e^s / (1.6·N), s ~ N(0, 1), and losing it moves the output by that weight times |v − out| ≤ ~3, while
# the bfloat16 allowance 2u·A is about 6e-3: one given row is visible only if its weight is above ~2e-3, which
# at N ≈ 2000 and 4 to 16 queries (the T = 1 steps) no scaling of the queries brings about (a larger scale
# makes the softmax peakier, on rows that are not the one in question; tests/test_attn_bound_host.py has the
# figures; at float16, with u 8 times smaller, plain draws would do).  So each query is a draw of standard deviation QMUL plus BETA times the keys, in its kv head, of the
# rows where a kernel's index can be off by one: the last kept row, a kept row in the middle, its own token's
# tail row (the last it sees) and the next token's (the first it must not see).  Each of these then leads
# the average row by BETA·|k|²/√D ≈ 3 nats (a weight of a few per cent) — what a model does
# anyway, where a token attends to itself and to recent context.
QMUL = 1.0
BETA = 0.25


def plant_boundaries(q, K, n, tk, nt, Hkv, dtype, beta=BETA):
    """q [Hq, T, D] + beta · (K[n − 1] + K[n // 2] + tk[vis(t) − 1] + tk[vis(t)]) per kv head, rounded to `dtype`
    (a torch dtype) and returned in q's own; K [>= n, Hkv·D] the kept keys, tk [>= nt, Hkv·D] the tail's.  A row
    that does not exist (no kept row, vis(t) = 0, vis(t) = nt) is left out."""
    Hq, T, D = q.shape
    G = Hq // Hkv
    add = torch.zeros(Hkv, T, D, dtype=torch.float64, device=q.device)
    if n > 0:
        add += (K[n - 1].double() + K[n // 2].double()).view(Hkv, 1, D)
    vis = visible(T, nt, q.device)
    tkd = tk[:nt].double().view(nt, Hkv, D)
    own = vis > 0
    add[:, own] += tkd[vis[own] - 1].transpose(0, 1)
    nxt = vis < nt
    add[:, nxt] += tkd[vis[nxt]].transpose(0, 1)
    out = q.double().view(Hkv, G, T, D) + beta * add[:, None]
    return out.view(Hq, T, D).to(dtype).to(q.dtype)


def attend(X, Y, seen, q, Hkv, scale, weights=None, mult=None):
    """float64 softmax(q_t·Xᵀ·scale)·Y over the keys seen[t] (bool [T, N]); X, Y [N, Hkv·D], q [Hq, T, D].
    Returns Ref(out, A), A the same weights on |Y|; a query that sees no key gives zeros.
    weights: a torch dtype to round exp(s − max) to before the products, the row sum staying unrounded
    (what extend.hip computes); mult [N]: how many times each key is counted (1 everywhere by default)."""
    Hq, T, D = q.shape
    G, N = Hq // Hkv, X.shape[0]
    if N == 0:
        z = torch.zeros(Hq, T, D, dtype=torch.float64, device=q.device)
        return Ref(z, z.clone())
    Xf, Yf = X.double().view(N, Hkv, D), Y.double().view(N, Hkv, D)
    s = torch.einsum("hgtd,nhd->hgtn", q.double().view(Hkv, G, T, D), Xf) * scale
    s = s.masked_fill(~seen, float("-inf"))
    m = s.amax(dim=-1, keepdim=True)
    e = torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))   # 0 where not seen
    if mult is not None:
        e = e * mult.double()
    den = e.sum(dim=-1, keepdim=True)
    den = torch.where(den > 0, den, torch.ones_like(den))
    w = (e if weights is None else e.to(weights).double()) / den
    out = torch.einsum("hgtn,nhd->hgtd", w, Yf).reshape(Hq, T, D)
    A = torch.einsum("hgtn,nhd->hgtd", w, Yf.abs()).reshape(Hq, T, D)
    return Ref(out, A)


def chunk_reference(k2, v2, rows, tk, tv, trows, q, Hkv, scale):
    """Ref per (b, t) over cat(K'/V'[:rows[b]], tail[:vis(b, t)]), q [B, Hq, T, D]; counts clamped to the
    tail's capacity as the kernels clamp them."""
    B, Hq, T, D = q.shape
    cap = tk.shape[1]
    outs, As = [], []
    for b in range(B):
        n, nb = int(rows[b]), min(max(int(trows[b]), 0), cap)
        X, Y = torch.cat([k2[b, :n], tk[b, :nb]]), torch.cat([v2[b, :n], tv[b, :nb]])
        seen = torch.arange(n + nb, device=q.device)[None, :] < (n + visible(T, nb, q.device))[:, None]
        r = attend(X, Y, seen, q[b], Hkv, scale)
        outs.append(r.out)
        As.append(r.A)
    return Ref(torch.stack(outs), torch.stack(As))


def bound(ref, vmax, dtype):
    return RTOL * ref.out.abs() + ATOL * vmax + 2 * U[dtype] * ref.A


def worst_ratio(out, ref, vmax, dtype):
    """max |out − ref| / bound over all elements (nan if out holds one)."""
    if out.numel() == 0:
        return 0.0
    return ((out.double() - ref.out).abs() / bound(ref, vmax, dtype)).max().item()


def check_bound(out, ref, vmax, dtype, what=""):
    assert out.shape == ref.out.shape, (out.shape, ref.out.shape)
    assert torch.isfinite(out).all()
    r = worst_ratio(out, ref, vmax, dtype)
    print(f"{what} {dtype}: worst |err| / bound {r:.3f}  (vmax {vmax:.3f}, max A {ref.A.max().item():.3f})")
    assert r <= 1.0, f"{what}: |out - ref| is {r:.3f} of the bound at its worst element"
    return r


# ------------------------------------------------------------------ the exact map of a one-hot tail
def onehot_tail(B, cap, Hkv, D, dtype, counts, device, spare=0):
    """A tail with zero keys and V[b, u, h, :] = onehot(u mod D) in its first counts[b] rows and NaN in
    every other row, as a [B, cap] view of [B, cap + spare] buffers (spare > 0: a strided batch)."""
    F = Hkv * D
    tk = torch.full((B, cap + spare, F), float("nan"), dtype=dtype, device=device)
    tv = torch.full((B, cap + spare, F), float("nan"), dtype=dtype, device=device)
    for b, n in enumerate(counts):
        u = torch.arange(n, device=device)
        tk[b, :n] = 0
        tv[b, :n] = torch.nn.functional.one_hot(u % D, D).to(dtype).repeat(1, Hkv)
    return tk[:, :cap], tv[:, :cap]


def onehot_expected(vis, D):
    """(count, vis) int64 [.., D] and [.., 1]: count[.., c] = #{u < vis : u mod D = c}.  Every logit is 0,
    every weight exactly 1 and every sum a small integer, so a kernel's output is count / vis in fp32."""
    vis = torch.as_tensor(vis, dtype=torch.int64)[..., None]
    c = torch.arange(D, dtype=torch.int64, device=vis.device)
    return (vis - c + D - 1).clamp(min=0) // D, vis


def check_onehot(out, vis, what=""):
    """out [.., D] fp32 against count / vis: zeros exactly zero, the rest within one float32 ulp of
    float32(count) / float32(vis) (the kernels divide in fp32; hardware division may be one ulp off).
    vis broadcasts against out's leading dimensions."""
    D = out.shape[-1]
    count, vis = onehot_expected(vis.to(out.device), D)
    count, vis = count.expand(out.shape), vis.expand(*out.shape[:-1], 1)
    exp = torch.where(count > 0, count.float() / vis.clamp(min=1).float(), torch.zeros((), device=out.device))
    zero = count == 0
    ulp = torch.nextafter(exp, torch.full_like(exp, float("inf"))) - exp
    bad = torch.where(zero, out != 0, ~((out - exp).abs() <= ulp))   # a NaN is bad either way
    if bad.any():
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} wrong elements, first at {i}: got {out[tuple(i)].item()!r}, "
                             f"expected {int(count[tuple(i)])} / {int(vis[tuple(i[:-1])])}")
