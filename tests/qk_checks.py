"""What the fused-importance tests share (import-only, like tests/attn_checks.py): synth inputs already rounded
to the dtype, float64 references of the row log-sum-exp and of K1's prompt-attention mass A, a first-order
per-row bound on each with its terms kept apart, the exact count maps of zero keys, and the calls into
librtkv.so with NaN guard regions behind the outputs.

References.  With x = scale·q·k in float64 from the rounded values (scale = the float32 the kernel is handed),
over the keys a row sees (j < Sk, j ≤ row0 + i when causal, key bias not −inf):

    lse64[b, h, i] = log Σ_j exp(x_j)                         (−inf for a row that sees no key)
    lse_in         = lse64 rounded once to float32            (what K1' is handed: K1' is judged alone)
    A64[b, i]      = (1/H) Σ_h Σ_{p < P, seen} exp(x_p − lse_in)      (P/S for a row that sees no key)

Bounds, first order in u = 2⁻²⁴, T = Σ_d |q_d||k_d|, w the float64 weight exp(x − lse_in), p_j the softmax:

    bound_A[b, i]      = u·[ (1/H) Σ_{h,p} w·(c_D·scale·T + 2|x| + 2|lse_in| + 4) + H·P·A64 ]
    bound_lse[b, h, i] = u·[ Σ_j p_j·(c_D·scale·T_j + 2|x_j|) + n_i + 4·max(1, |lse64|) ]

term by term: `dot` — the fp32 accumulation of the D products moves x by at most c_D·u·scale·T, and w by that
times w; `x` — the fma x·(scale·log₂e) − lse·log₂e rounds scale·log₂e, the product lse·log₂e and the result,
each relative to |x| or |lse| (`lse`), in units of the exponent, where an absolute error δ is a relative error
δ of w; `const` — the hardware exp2 (1 ulp), the final division by H and the conversions; `sum` — H·P fp32
additions of non-negative terms, each rounding at most u times the running sum ≤ H·A64.  For the lse: the
same `dot` and `x` terms weighted by the softmax (d lse = Σ p_j dx_j), `n` — n_i additions relative to the sum,
i.e. n_i·u absolute in the logarithm, and `const` — log2 and the multiply by ln 2, relative to |lse|.

c_D.  float16 and bfloat16: a product of two 11-bit (8-bit) significands is exact in fp32, only the D
accumulations round: c_D = D.  float32 (attn_f32.hip, split3): x = h + l + ll with h = bf16(x), l = bf16(x − h),
ll = bf16(x − h − l); |x − h| ≤ 2⁻⁸|x| (half a bf16 ulp), |x − h − l| ≤ 2⁻¹⁶|x|, and that residual is a multiple
of x's last bit 2⁻²³·2ᵉ no larger than 2⁻¹⁶·2ᵉ, i.e. at most 8 significant bits: ll is exact and so is the
three-way split.  Of the nine part products six are kept (h·h, h·l, l·h, h·ll, ll·h, l·l), each exact in fp32;
the dropped l·ll, ll·l, ll·ll are at most (2·2⁻²⁴ + 2⁻³²)·|q_d||k_d| — 2.01·u·T per dot product.  The kept ones
are 6·D fp32 accumulations whose running absolute sum is at most T·(1 + 2·2⁻⁸ + 2·2⁻¹⁶ + 2⁻¹⁶), so

    c_D(float32) = 6·D·(1 + 2⁻⁷ + 2⁻¹⁴) + 2.01            (776.1 at D = 128).

The exact f32-MFMA kernels (RTKV_LSE_F32_EXACT: D rounded products, D accumulations, c = 2·D) lie inside it.

Count maps.  With zero keys (and lse_in = 0) every logit is 0 and every weight exactly 1, whatever the
queries: K1' must return min(P, row0 + i + 1) (causal) or P bit for bit — the head sums are small integers
and (cnt·H)/H is exact — and the LSE ln(n_i) within 4·2⁻²³·max(1, ln n_i) (an exact sum, one hardware log2,
one multiply); with a key padding the counts leave the padded keys out, and a row that counts none holds 0 (−inf).  The nearest wrong count differs by more than 1/(n_i + 1) ≥ 1e-4 relative for every S used.

tests/test_qk_bound_host.py shows on the CPU that a float32 model of a correct kernel stays far inside these
bounds and that off-by-one kernels do not."""
import ctypes
import functools
import math
from collections import namedtuple

import numpy as np
import torch

import synth

U = 2.0 ** -24
TD = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
GUARD = 64          # NaN elements behind every output
LOG2E_F32 = float(np.float32(1.4426950408889634))

_CASE_FIELDS = "kind dtype B H Hkv S D P causal row0 pad boost seed"
Case = namedtuple("Case", _CASE_FIELDS, defaults=("k1", "float16", 1, 1, 1, 64, 128, 16, True, 0, None, None, 0))
Case.__doc__ = """kind: 'k1' (K1', P prompt columns) or 'lse'.  S query rows at global rows row0 .. row0 + S − 1.
pad: None or (left, right) — per batch row, leading and trailing padding keys (a −inf key bias).
boost: None or (key row, ((first, last query row), ..)) — that key and those queries set to 4.0, a logit
about 180 above the row's first one (the overflow of attn_lse32.hip's unchecked sum)."""


def case_id(c):
    s = f"{c.dtype}-B{c.B}-H{c.H}/{c.Hkv}-S{c.S}-D{c.D}"
    if c.kind == "k1":
        s += f"-P{c.P}"
    if not c.causal:
        s += "-full"
    if c.row0:
        s += f"-row0={c.row0}"
    if c.pad:
        s += "-pad" + "/".join(",".join(map(str, p)) for p in c.pad)
    if c.boost:
        s += "-boost"
    return s


def freeze(c):
    """A Case read back from JSON: lists → tuples (hashable again)."""
    def tup(v):
        return tuple(tup(e) for e in v) if isinstance(v, (list, tuple)) else v
    return Case(*[tup(v) for v in c])


def scale_of(D):
    return float(np.float32(1.0 / math.sqrt(D)))   # the float32 the kernel is handed


def c_dot(dtype, D):
    return 6 * D * (1 + 2.0 ** -7 + 2.0 ** -14) + 2.01 if dtype == "float32" else float(D)


def keys_len(c):
    """Key rows the case holds: every row a query may see and the P prompt rows."""
    return max(c.row0 + c.S, c.P) if c.kind == "k1" else c.S


# ------------------------------------------------------------------------------------------------ inputs
Inputs = namedtuple("Inputs", "Q K bias")   # numpy storage: Q [B, H, S, D], K [B, Sk, Hkv·D], bias [B, Sk] fp32 or None


@functools.lru_cache(maxsize=8)
def inputs(c, zero_keys=False):
    """The case's synth draws in the dtype's storage (uint16 bit patterns for the half types), so the CPU and
    the GPU tests see the same bits.  zero_keys: the count map's keys."""
    Sk = keys_len(c)
    seed = 7919 * c.seed + 31 * c.S + c.H + 1000 * c.D + c.P
    q = synth.normal(seed, (c.B, c.H, c.S, c.D), 11)
    k = synth.normal(seed, (c.B, Sk, c.Hkv * c.D), 12)
    if zero_keys:
        k = np.zeros_like(k)
    elif c.boost:
        key, rows = c.boost
        k[:, key] = 4.0
        for a, z in rows:
            q[:, :, a:z + 1] = 4.0
    bias = None
    if c.pad:
        assert Sk == c.S, "a key bias is [B, S]: the case needs P <= S and row0 = 0"
        bias = np.zeros((c.B, Sk), np.float32)
        for b in range(c.B):
            bias[b, :c.pad[0][b]] = -np.inf
            if c.pad[1][b]:
                bias[b, Sk - c.pad[1][b]:] = -np.inf
    return Inputs(synth.cast(q, c.dtype), synth.cast(k, c.dtype), bias)


def f64(stored, dtype):
    return torch.from_numpy(synth.to_f32(stored, dtype).astype(np.float64))


def seen_keys(c, b, bias=None):
    """bool [S, Sk]: the keys row i of batch row b sees."""
    Sk = keys_len(c)
    j = torch.arange(Sk)[None, :]
    i = torch.arange(c.S)[:, None]
    seen = (j <= c.row0 + i) if c.causal else torch.ones(c.S, Sk, dtype=torch.bool)
    if bias is not None:
        seen = seen & torch.from_numpy(np.isfinite(bias[b]))[None, :]
    return seen


# -------------------------------------------------------------------------------------------- references
Logits = namedtuple("Logits", "x T seen")                      # per batch row: [H, S, Sk] float64 ×2, [S, Sk] bool
LseRef = namedtuple("LseRef", "lse lse_in bound terms n")      # [B, H, S]; terms: dict of [B, H, S]
ARef = namedtuple("ARef", "A bound terms dead")                # [B, S]; dead: rows that see no key


def logits(c, inp, b, cols=None):
    """x = scale·q·k and T = Σ|q||k| in float64 for batch row b, over the first `cols` keys (all by default)."""
    Sk = keys_len(c) if cols is None else cols
    g = c.H // c.Hkv
    q = f64(inp.Q[b], c.dtype).view(c.Hkv, g, c.S, c.D)
    k = f64(inp.K[b, :Sk], c.dtype).view(Sk, c.Hkv, c.D)
    x = torch.einsum("hgid,jhd->hgij", q, k).reshape(c.H, c.S, Sk) * scale_of(c.D)
    T = torch.einsum("hgid,jhd->hgij", q.abs(), k.abs()).reshape(c.H, c.S, Sk)
    return Logits(x, T, seen_keys(c, b, inp.bias)[:, :Sk])


@functools.lru_cache(maxsize=None)
def lse_reference(c, with_bound=True):
    inp = inputs(c)
    sc, cd = scale_of(c.D), c_dot(c.dtype, c.D)
    out, bnd, ns = [], [], []
    terms = {k: [] for k in ("dot", "x", "n", "const")}
    for b in range(c.B):
        x, T, seen = logits(c, inp, b)
        xm = x.masked_fill(~seen, float("-inf"))
        lse = torch.logsumexp(xm, dim=-1)
        n = seen.sum(-1).double()[None, :].expand(c.H, c.S)
        out.append(lse)
        ns.append(n)
        if with_bound:
            p = torch.exp(xm - torch.where(torch.isfinite(lse), lse, torch.zeros_like(lse))[..., None])
            terms["dot"].append(U * cd * sc * (p * T).sum(-1))
            terms["x"].append(U * 2 * (p * x.abs()).sum(-1))
            terms["n"].append(U * n)
            terms["const"].append(U * 4 * lse.abs().clamp(min=1.0))
    lse = torch.stack(out)
    terms = {k: torch.stack(v) for k, v in terms.items()} if with_bound else {}
    bound = sum(terms.values()) if with_bound else None
    return LseRef(lse, lse.float(), bound, terms, torch.stack(ns))


@functools.lru_cache(maxsize=None)
def a_reference(c):
    """A64 and its bound, from lse_in = float32(lse64) of the same case over all its keys."""
    inp = inputs(c)
    sc, cd = scale_of(c.D), c_dot(c.dtype, c.D)
    lse_in = lse_reference(c, with_bound=False).lse_in
    As, deads = [], []
    terms = {k: [] for k in ("dot", "x", "lse", "const", "sum")}
    for b in range(c.B):
        x, T, seen = logits(c, inp, b, cols=c.P)
        li = lse_in[b].double()
        dead = torch.isneginf(li)                                      # [H, S]
        w = torch.exp(x - torch.where(dead, torch.zeros_like(li), li)[..., None])
        w = torch.where(seen[None] & ~dead[..., None], w, torch.zeros_like(w))
        rows = torch.where(dead, torch.full_like(li, c.P / c.S), w.sum(-1))
        A = rows.mean(0)
        As.append(A)
        deads.append(dead.all(0))
        assert bool((dead.all(0) == dead.any(0)).all()), "a row sees no key in every head or in none"
        terms["dot"].append(U * cd * sc * (w * T).sum((0, 2)) / c.H)
        terms["x"].append(U * 2 * (w * x.abs()).sum((0, 2)) / c.H)
        terms["lse"].append(U * 2 * (w * li.abs().masked_fill(dead, 0)[..., None]).sum((0, 2)) / c.H)
        terms["const"].append(U * 4 * w.sum((0, 2)) / c.H)
        terms["sum"].append(U * c.H * c.P * A)
    terms = {k: torch.stack(v) for k, v in terms.items()}
    return ARef(torch.stack(As), sum(terms.values()), terms, torch.stack(deads))


def dead_row_value(c):
    """What a row that sees no key must hold: the head mean of float32(P)/float32(S) as the reduce kernel forms
    it (H equal fp32 terms added in order, one division) — P/S to within an ulp or two, and bit for bit this."""
    v = np.float32(c.P) / np.float32(c.S)
    s = np.float32(0)
    for _ in range(c.H):
        s = np.float32(s + v)
    return float(np.float32(s / np.float32(c.H)))


# ---------------------------------------------------------------------------------------------- checking
def _worst(err, bound, terms):
    # a bound of 0 (no visible prompt column: every weight is exactly 0) admits no error at all
    r = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    r = torch.where(torch.isnan(err), torch.full_like(r, float("inf")), r)
    at = int(r.argmax())
    idx = np.unravel_index(at, tuple(r.shape))
    lead = max(terms, key=lambda k: float(terms[k][idx]))
    parts = "  ".join(f"{k} {float(v[idx]):.2e}" for k, v in terms.items())
    return float(r.max()), idx, lead, parts


def a_ratio(A, ref):
    """worst |A − A64| / bound over the rows that see a key, where, the leading term there, all terms there."""
    live = ~ref.dead
    err = torch.where(live, (A.double() - ref.A).abs(), torch.zeros_like(ref.A))
    return _worst(err, ref.bound, ref.terms)


def check_A(A, c, what=""):
    """K1's A [B, S] (fp32, CPU) against the float64 reference: finite, every row within its bound, rows that see
    no key exactly the uniform row.  Returns worst error/bound."""
    ref = a_reference(c)
    assert tuple(A.shape) == (c.B, c.S), A.shape
    assert torch.isfinite(A).all(), f"{what} {case_id(c)}: A holds a NaN or an inf"
    r, idx, lead, parts = a_ratio(A, ref)
    print(f"{what} {case_id(c)}: worst |A - A64| / bound {r:.4f} at {idx} (A64 {float(ref.A[idx]):.3e}, "
          f"bound {float(ref.bound[idx]):.2e}, leading term {lead}: {parts})")
    assert r <= 1.0, f"{what} {case_id(c)}: |A - A64| is {r:.3f} of the bound at {idx}; terms {parts}"
    if ref.dead.any():
        assert bool((A[ref.dead] == dead_row_value(c)).all()), f"{what} {case_id(c)}: a row that sees no key is not P/S"
        assert abs(dead_row_value(c) - c.P / c.S) <= 4 * U * c.P / c.S
    return r


def lse_ratio(lse, ref):
    live = torch.isfinite(ref.lse)
    err = torch.where(live, (lse.double() - ref.lse).abs(), torch.zeros_like(ref.lse))
    return _worst(err, ref.bound, ref.terms)


def check_lse(lse, c, what=""):
    ref = lse_reference(c)
    assert tuple(lse.shape) == (c.B, c.H, c.S), lse.shape
    live = torch.isfinite(ref.lse)
    assert torch.isfinite(lse[live]).all(), f"{what} {case_id(c)}: lse holds a NaN or an inf"
    assert torch.isneginf(lse[~live]).all(), f"{what} {case_id(c)}: a row that sees no key is not -inf"
    r, idx, lead, parts = lse_ratio(lse, ref)
    print(f"{what} {case_id(c)}: worst |lse - lse64| / bound {r:.4f} at {idx} (lse64 {float(ref.lse[idx]):.4f}, "
          f"bound {float(ref.bound[idx]):.2e}, leading term {lead}: {parts})")
    assert r <= 1.0, f"{what} {case_id(c)}: |lse - lse64| is {r:.3f} of the bound at {idx}; terms {parts}"
    return r


# ------------------------------------------------------------------------------------------- count maps
def counts(c):
    """int64 [B, S]: the keys (k1: prompt columns) row i sees; padding keys are not seen."""
    n = c.P if c.kind == "k1" else c.S
    bias = inputs(c, True).bias
    return torch.stack([seen_keys(c, b, bias)[:, :n].sum(-1) for b in range(c.B)])


def check_count_A(A, c, what=""):
    exp = counts(c).float()
    bad = ~(A == exp)
    if bad.any():
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what} {case_id(c)}: {int(bad.sum())} wrong counts, first at {i}: got "
                             f"{A[tuple(i)].item()!r}, expected {exp[tuple(i)].item()}")


def check_count_lse(lse, c, what=""):
    """Returns the worst error in units of 2⁻²³·max(1, ln n); a row that sees no key must hold −inf."""
    n = counts(c)[:, None, :].expand(c.B, c.H, c.S)
    exp = n.double().log()
    live = n > 0
    ulps = torch.where(live, (lse.double() - exp).abs() / (2.0 ** -23 * exp.clamp(min=1.0)), torch.zeros_like(exp))
    bad = torch.where(live, ~(ulps <= 4.0), ~torch.isneginf(lse))
    if bad.any():
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what} {case_id(c)}: {int(bad.sum())} rows off, first at {i}: got "
                             f"{lse[tuple(i)].item()!r}, expected ln {int(n[tuple(i)])} = {exp[tuple(i)].item()!r}")
    return float(ulps.max())


# ----------------------------------------------------------------------------------- the library calls
def to_device(stored, dtype, device="cuda"):
    if dtype == "float32":
        return torch.from_numpy(np.ascontiguousarray(stored)).to(device)
    return torch.from_numpy(np.ascontiguousarray(stored).view(np.int16)).to(device).view(TD[dtype])


def guarded(shape, device="cuda", row_pad=1):
    """(view, whole buffer): an fp32 output of `shape` in a NaN-filled buffer with GUARD NaN elements behind it;
    row_pad > 1 pads the last dimension's stride to a multiple of it (NaN in the gaps)."""
    last = -(-shape[-1] // row_pad) * row_pad
    n = int(np.prod(shape[:-1])) * last
    buf = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=device)
    view = buf[:n].view(*shape[:-1], last)[..., :shape[-1]]
    return view, buf


def assert_guard(buf, view, what):
    n = buf.numel() - GUARD
    assert torch.isnan(buf[n:]).all(), f"{what}: the {GUARD} elements behind the output were written"
    if view.shape[-1] != view.stride(-2):
        gaps = buf[:n].view(-1, view.stride(-2))[:, view.shape[-1]:]
        assert torch.isnan(gaps).all(), f"{what}: the padding between rows was written"


def device_operands(c, inp, layout="bsf"):
    """Q [B, H, S, D] and the keys on the device.  layout: 'bsf' (keys [B, Sk, Hkv·D]), 'bhsd' (keys
    [B, Hkv, Sk, D]) or 'q_bshd' (bsf keys, Q the transposed view of a [B, S, H, D] tensor: q_stride_s = H·D)."""
    Q = to_device(inp.Q, c.dtype)
    K = to_device(inp.K, c.dtype)
    if layout == "bhsd":
        K = K.view(c.B, K.shape[1], c.Hkv, c.D).permute(0, 2, 1, 3).contiguous()
    elif layout == "q_bshd":
        Q = Q.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
        assert Q.stride(2) == c.H * c.D and Q.stride(1) == c.D
    bias = None if inp.bias is None else torch.from_numpy(inp.bias).cuda()
    return Q, K, bias


def run_k1(c, inp, lse_in, layout="bsf", stages=None):
    """rtkv_importance_qk_lse_ws as engine.importance_qk_lse calls it (stages: a HipShardStages, whose
    aggregate_qk then makes the call), A and lse_in in guarded buffers (lse rows padded to 16 bytes, which the
    entry point requires of an S that is no multiple of 4).  Returns A [B, S] on the CPU."""
    from rtkv import _lib as L
    from rtkv.engine import qk_desc
    Q, K, bias = device_operands(c, inp, layout)
    lse, lse_buf = guarded((c.B, c.H, c.S), row_pad=4)
    lse.copy_(lse_in)
    A, A_buf = guarded((c.B, c.S))
    k_layout = "bhsd" if layout == "bhsd" else "bsf"
    if stages is not None:
        assert k_layout == "bsf" and bias is None
        stages.aggregate_qk(Q, K[:, :c.P].contiguous(), lse, c.P, c.row0, c.causal, A)
    else:
        qd = qk_desc(Q, K, lse, causal=c.causal, k_layout=k_layout, row0=c.row0, key_bias=bias)
        scratch = torch.empty(int(L.lib().rtkv_qk_scratch_size(qd.B, qd.H, qd.S)), dtype=torch.uint8, device="cuda")
        L.check(L.lib().rtkv_importance_qk_lse_ws(ctypes.byref(qd), int(c.P), A.data_ptr(), scratch.data_ptr(),
                                                  scratch.numel(), L.stream_ptr(Q.device)), "rtkv_importance_qk_lse_ws")
    torch.cuda.synchronize()
    assert_guard(A_buf, A, f"K1' {case_id(c)}")
    return A.cpu()


def run_lse(c, inp, layout="bsf"):
    """rtkv_attention_lse as engine.attention_lse calls it, the output in a guarded buffer."""
    from rtkv import _lib as L
    from rtkv.engine import qk_desc
    Q, K, bias = device_operands(c, inp, layout)
    lse, buf = guarded((c.B, c.H, c.S))
    qd = qk_desc(Q, K, lse, causal=c.causal, k_layout="bhsd" if layout == "bhsd" else "bsf", key_bias=bias)
    L.check(L.lib().rtkv_attention_lse(ctypes.byref(qd), lse.data_ptr(), L.stream_ptr(Q.device)), "rtkv_attention_lse")
    torch.cuda.synchronize()
    assert_guard(buf, lse, f"lse {case_id(c)}")
    return lse.cpu()


def run_case(c, stages=None):
    """{'out', 'count'}: the library's result on the case's random data and on its count map (zero keys and, for
    K1', lse_in = 0; the padding stays)."""
    if c.kind == "k1":
        return {"out": run_k1(c, inputs(c), lse_reference(c, with_bound=False).lse_in, stages=stages),
                "count": run_k1(c, inputs(c, True), torch.zeros(c.B, c.H, c.S), stages=stages)}
    return {"out": run_lse(c, inputs(c)), "count": run_lse(c, inputs(c, True))}


def check_case(c, outs, what=""):
    """(worst error/bound, worst count-map error in ulps — 0 for K1', which is exact)."""
    if c.kind == "k1":
        check_count_A(outs["count"], c, what)
        return check_A(outs["out"], c, what), 0.0
    ulps = check_count_lse(outs["count"], c, what)
    return check_lse(outs["out"], c, what), ulps
