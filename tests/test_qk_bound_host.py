"""CPU: the per-row bounds and count maps of tests/qk_checks.py can tell a right fused-importance kernel from a
wrong one, before any GPU run (as tests/test_attn_bound_host.py does for the chunk attention).

The "correct kernel" is a float32 model of what the HIP kernels compute, no library call: a float32 dot
product, exp2(fma(x, scale·log₂e, −lse·log₂e)), float32 sums in the kernel's order (prompt columns, then
heads) and one division by H; for the LSE a float32 dot, exp2 against the row maximum summed in key order,
log2 and a multiply.  It does not imitate the matrix core's accumulation order.  The model must stay within
half of the bound at every case and dtype; every mutant — an off-by-one prompt length or diagonal, the wrong
kv head, a head left out, a neighbour's lse, a tile's last row reading the clamped query, a key dropped or
counted twice — must exceed it wherever it changes the result at all, and where a case cannot see a mutant
(no grouped heads, no causal mask, a single 64-row tile) the test asserts that its output is unchanged
bit for bit instead of skipping it.  The count maps get the same treatment at the (S, P, row0) of the GPU file."""
import numpy as np
import pytest
import torch

import synth
from qk_checks import (Case, LOG2E_F32, a_ratio, a_reference, case_id, check_count_A, check_count_lse, inputs,
                       lse_ratio, lse_reference, scale_of)

K1_MUTANTS = ("P-1", "diag-1", "diag+1", "gqa", "head", "lse", "tile")
LSE_MUTANTS = ("last", "diag", "edge")

# H/Hkv, S, D, P, causal, row0: the cases the bound form was tried at (one without a causal mask, one without
# grouped heads, one at head_dim 32, the largest at P = 128) and two sequence-shard rows
K1_SHAPES = [
    (8, 2, 300, 128, 60, True, 0),
    (4, 2, 132, 64, 26, False, 0),
    (43, 43, 132, 128, 26, True, 0),
    (6, 2, 68, 32, 13, True, 0),
    (8, 4, 700, 128, 128, True, 0),
    (6, 2, 64, 64, 60, True, 37),
    (4, 2, 132, 128, 128, True, 100),
]
LSE_SHAPES = [s for s in K1_SHAPES if s[6] == 0]


def _cases(shapes, kind):
    out = []
    for H, Hkv, S, D, P, causal, row0 in shapes:
        for dt in ("float16", "bfloat16", "float32"):
            if dt == "float32" and D != 128:
                continue   # the fp32 kernels are head_dim 128 only
            out.append(Case(kind=kind, dtype=dt, B=1, H=H, Hkv=Hkv, S=S, D=D, P=P, causal=causal, row0=row0))
    return out


def _f32(stored, dtype):
    return synth.to_f32(stored, dtype)


def expect_change(c, mut):
    """Whether the mutant can change anything at this case (else its output must be bit-identical)."""
    return {
        "P-1": (not c.causal) or c.row0 + c.S >= c.P,          # some row sees column P − 1
        "diag-1": c.causal and c.row0 <= c.P - 1,              # row 0's diagonal is a prompt column
        "diag+1": c.causal and c.row0 + 1 <= c.P - 1,
        "gqa": c.H // c.Hkv > 1 and c.Hkv > 1,
        "head": True,
        "lse": True,
        "tile": c.S > 64,                                      # a row 63 that is not row S − 1
        "last": True,
        "diag": c.causal,
        "edge": c.S > 64,
    }[mut]


def model_k1(c, Q, K, lse_in, mut=None):
    """float32 model of K1' on batch row 0.  Q [H, S, D], K [Sk, Hkv·D] float32 values, lse_in [H, S] float32."""
    H, S, D, P, g = c.H, c.S, c.D, c.P, c.H // c.Hkv
    Kh = K[:P].reshape(P, c.Hkv, D)
    heads = [(h % c.Hkv) if mut == "gqa" else h // g for h in range(H)]
    if mut == "tile":
        Q = Q.copy()
        rows = [i for i in range(63, S - 1, 64)]
        Q[:, rows] = Q[:, S - 1:S]
    if mut == "lse":
        lse_in = np.concatenate([lse_in[:, 1:], lse_in[:, S - 2:S - 1]], axis=1)
    sc = np.float64(np.float32(np.float32(scale_of(D)) * np.float32(LOG2E_F32)))
    nl2 = (-lse_in * np.float32(LOG2E_F32)).astype(np.float32)
    Pe = P - 1 if mut == "P-1" else P
    shift = {"diag-1": -1, "diag+1": 1}.get(mut, 0)
    i = np.arange(S)[:, None]
    p = np.arange(P)[None, :]
    ok = (p < Pe) & ((p <= c.row0 + i + shift) if c.causal else True)
    tot = np.zeros(S, np.float32)
    for h in range(H):
        if mut == "head" and h == H - 1:
            continue
        x = Q[h] @ Kh[:, heads[h]].T                                              # float32 dot
        w = np.exp2((x.astype(np.float64) * sc + nl2[h][:, None]).astype(np.float32))   # one rounding: the fma
        hs = np.zeros(S, np.float32)
        for col in range(P):
            hs += np.where(ok[:, col], w[:, col], np.float32(0))
        tot += hs
    return torch.from_numpy(tot / np.float32(H))[None]


def model_lse(c, Q, K, mut=None):
    """float32 model of the LSE on batch row 0: [1, H, S]."""
    H, S, D, g = c.H, c.S, c.D, c.H // c.Hkv
    Kh = K.reshape(S, c.Hkv, D)
    i = np.arange(S)[:, None]
    j = np.arange(S)[None, :]
    mult = ((j <= i) if c.causal else np.ones((S, S), bool)).astype(np.float32)
    if mut == "last":
        mult[:, S - 1] = 0
    elif mut == "diag" and c.causal:
        mult[np.arange(S), np.arange(S)] = 0
    elif mut == "edge" and S > 64:
        mult[:, 64] *= 2
    sc = np.float64(np.float32(np.float32(scale_of(D)) * np.float32(LOG2E_F32)))
    out = np.empty((H, S), np.float32)
    for h in range(H):
        x = Q[h] @ Kh[:, h // g].T
        xm = np.where(mult > 0, x, -np.inf).astype(np.float32)
        M = (xm.max(axis=1).astype(np.float64) * sc).astype(np.float32)
        Mf = np.where(np.isfinite(M), M, np.float32(0))
        e = np.exp2((xm.astype(np.float64) * sc - Mf[:, None]).astype(np.float32))
        l = np.zeros(S, np.float32)
        for col in range(S):
            l += mult[:, col] * e[:, col]
        with np.errstate(divide="ignore"):
            out[h] = ((Mf + np.log2(l)) * np.float32(0.6931471805599453)).astype(np.float32)
    return torch.from_numpy(out)[None]


@pytest.mark.parametrize("c", _cases(K1_SHAPES, "k1"), ids=case_id)
def test_a_bound_tells_right_from_wrong(c):
    inp, ref = inputs(c), a_reference(c)
    Q, K = _f32(inp.Q[0], c.dtype), _f32(inp.K[0], c.dtype)
    lse_in = lse_reference(c, with_bound=False).lse_in[0].numpy()
    right = model_k1(c, Q, K, lse_in)
    r = a_ratio(right, ref)
    rel = float((ref.bound / ref.A).min()), float((ref.bound / ref.A).max())
    print(f"model {r[0]:.4f} of the bound (leading term {r[2]}); bound / A64 from {rel[0]:.1e} to {rel[1]:.1e}")
    assert r[0] <= 0.5, r
    left_out = 0
    for mut in K1_MUTANTS:
        out = model_k1(c, Q, K, lse_in, mut)
        if not expect_change(c, mut):
            assert torch.equal(out, right), f"{mut} should not be visible at {case_id(c)}"
            left_out += 1
            continue
        m = a_ratio(out, ref)[0]
        print(f"  {mut}: {m:.1f}")
        assert not m <= 1.0, (mut, m)
    assert left_out <= 2, left_out


@pytest.mark.parametrize("c", _cases(LSE_SHAPES, "lse"), ids=case_id)
def test_lse_bound_tells_right_from_wrong(c):
    inp, ref = inputs(c), lse_reference(c)
    Q, K = _f32(inp.Q[0], c.dtype), _f32(inp.K[0], c.dtype)
    right = model_lse(c, Q, K)
    r = lse_ratio(right, ref)
    print(f"model {r[0]:.4f} of the bound (leading term {r[2]}); bound from {float(ref.bound.min()):.1e} to "
          f"{float(ref.bound.max()):.1e}")
    assert r[0] <= 0.5, r
    left_out = 0
    for mut in LSE_MUTANTS:
        out = model_lse(c, Q, K, mut)
        if not expect_change(c, mut):
            assert torch.equal(out, right), f"{mut} should not be visible at {case_id(c)}"
            left_out += 1
            continue
        err = (out.double() - ref.lse).abs()
        m = float(torch.where(torch.isfinite(err), err / ref.bound, torch.full_like(err, float("inf"))).max())
        print(f"  {mut}: {m:.1f}")
        assert not m <= 1.0, (mut, m)
    assert left_out <= 2, left_out


# (S, P, row0) of tests/test_gpu_qk_variants.py: the sequence-shard rows and a few whole sequences
COUNT_K1 = [(S, 128, r) for S in (64, 132) for r in (1, 37, 63, 64, 100, 127, 128)] + \
           [(S, 60, r) for S in (64, 132) for r in (59, 60)] + \
           [(4, 1, 0), (61, 33, 0), (65, 64, 0), (257, 128, 0), (68, 97, 0), (130, 65, 0)]
COUNT_LSE = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 193, 255, 256, 257, 300)


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
def test_count_maps_tell_right_from_wrong(causal):
    """Zero keys, lse_in = 0: the model returns the counts exactly, and every mask mutant changes at least one
    count wherever the mask it breaks is in play."""
    for S, P, row0 in COUNT_K1:
        c = Case(kind="k1", dtype="float16", B=1, H=3, Hkv=3, S=S, D=32, P=P, causal=causal, row0=row0)
        inp = inputs(c, True)
        Q, K = _f32(inp.Q[0], c.dtype), _f32(inp.K[0], c.dtype)
        zero = np.zeros((c.H, S), np.float32)
        check_count_A(model_k1(c, Q, K, zero), c)
        for mut in ("P-1", "diag-1", "diag+1"):
            out = model_k1(c, Q, K, zero, mut)
            if expect_change(c, mut):
                with pytest.raises(AssertionError):
                    check_count_A(out, c)
            else:
                check_count_A(out, c)
    for S in COUNT_LSE:
        c = Case(kind="lse", dtype="float16", B=1, H=2, Hkv=2, S=S, D=64, causal=causal)
        inp = inputs(c, True)
        Q, K = _f32(inp.Q[0], c.dtype), _f32(inp.K[0], c.dtype)
        assert check_count_lse(model_lse(c, Q, K), c) <= 2.0
        for mut in LSE_MUTANTS:
            out = model_lse(c, Q, K, mut)
            if expect_change(c, mut):
                with pytest.raises(AssertionError):
                    check_count_lse(out, c)
            else:
                check_count_lse(out, c)
