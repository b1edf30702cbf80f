"""CPU: the per-element bound of tests/attn_checks.py can tell a right chunk-attention kernel from a wrong
one, at the inputs of tests/test_gpu_extend.py's ground-truth cases — and its exact one-hot map likewise.

float64 torch on the CPU, no library call: K, V, q and the tail are the synth draws of the GPU cases (same
seeds, same queries; the kept rows are the first 0.85·S unquantized rows, about what
the GPU file's layers keep).  The correct answer with its
weights rounded to the dtype relative to the row maximum, as extend.hip rounds them, must pass the bound;
each wrong kernel must fail it, at every (shape, dtype, step) of the GPU file — a mutant that passed here
could not be seen on the GPU either.

What this found about the inputs.  With plain N(0, 1) draws every mutant fails at float16 for query scales up
to 1.5 (lowest |err| / bound 1.2 to 1.6), but at bfloat16 no scaling of the queries makes every mutant fail: of
the 24 (shape, step) combinations a mutant passes the bound at 17 (query scale 0.5), 16 (0.75), 13 (1), 12 (1.5),
12 (2), 15 (3) and 19 (4), with ratios down to 0.1 to 0.2 — mostly the T = 1 and T = 2 steps and those over
~2000 rows, where one given row weighs about 5e-4 and few queries look at it.  A larger scale makes the
softmax peakier, but not on the row in question.  So the queries carry a multiple of the keys at the
places where an index can be off by one (attn_checks.plant_boundaries, BETA): then every mutant is at least
5.4 times the bound at bfloat16 and 41 times at float16, and the correct answer at most 0.1 of it."""
import numpy as np
import pytest
import torch

import synth
from attn_checks import (BETA, QMUL, SHAPES, STEPS, TD, attend, check_onehot, onehot_tail, plant_boundaries, visible,
                         worst_ratio)

CASES = [(s, dt, STEPS[i]) for i, s in enumerate(SHAPES) for dt in ("float16", "bfloat16")]

MUTANTS = ("vis+1", "vis-1", "last packed row missing", "last tail row of the last query missing",
           "one packed row twice")   # and "vis+1, the last query right" where T > 1


def draw(seed, shape, dtype, mul=1.0):
    stored = synth.cast(synth.normal(seed, shape) * np.float32(mul), dtype)
    return torch.from_numpy(synth.to_f32(stored, dtype).astype(np.float64))


def answers(S, Hkv, D, Hq, dtype, T, older, qmul=QMUL, beta=BETA):
    """(reference, {name: output}, vmax) — 'right' and every mutant, all with dtype-rounded weights."""
    F, n, nt = Hkv * D, int(0.85 * S), T + older
    K, V = synth.kv(S * 7 + Hkv, 1, n, F, dtype)       # layer()'s seed
    K, V = (torch.from_numpy(synth.to_f32(a, dtype).astype(np.float64))[0] for a in (K, V))
    q = draw(S + T, (1, Hq, T, D), dtype, qmul)[0]       # test_ground_truth's q and tail
    tk, tv = draw(S + 10 * nt, (nt + 3, F), dtype)[:nt], draw(S + 10 * nt + 1, (nt + 3, F), dtype)[:nt]   # make_tail
    q = plant_boundaries(q, K, n, tk, nt, Hkv, TD[dtype], beta)
    X, Y = torch.cat([K, tk]), torch.cat([V, tv])
    idx = torch.arange(n + nt)[None, :]
    vis = visible(T, nt)
    seen = idx < (n + vis)[:, None]
    scale, vmax = 1.0 / D ** 0.5, max(Y.abs().max().item(), 1.0)
    ref = attend(X, Y, seen, q, Hkv, scale)
    wd = TD[dtype]
    out = {"right": attend(X, Y, seen, q, Hkv, scale, weights=wd).out}
    # vis + 1: queries 0 .. T − 2 see the next token's row; the last one reads the row past the count, which is
    # NaN in every tail of the GPU file.  The others must give the kernel away without it (T > 1).
    early = attend(X, Y, idx < (n + (vis + 1).clamp(max=nt))[:, None], q, Hkv, scale, weights=wd).out
    if T > 1:
        out["vis+1, the last query right"] = torch.cat([early[:, :-1], out["right"][:, -1:]], dim=1)
    out["vis+1"] = torch.cat([early[:, :-1], torch.full_like(early[:, -1:], float("nan"))], dim=1)
    out["vis-1"] = attend(X, Y, idx < (n + (vis - 1).clamp(min=0))[:, None], q, Hkv, scale, weights=wd).out
    m = seen.clone()
    m[:, n - 1] = False
    out["last packed row missing"] = attend(X, Y, m, q, Hkv, scale, weights=wd).out
    m = seen.clone()
    m[T - 1, n + int(vis[T - 1]) - 1] = False
    out["last tail row of the last query missing"] = attend(X, Y, m, q, Hkv, scale, weights=wd).out
    mult = torch.ones(n + nt)
    mult[n // 2] = 2
    out["one packed row twice"] = attend(X, Y, seen, q, Hkv, scale, weights=wd, mult=mult).out
    return ref, out, vmax


@pytest.mark.parametrize("shape,dtype,steps", CASES, ids=[f"{s[0]}-{s[1]}-{s[3]}-{dt}" for s, dt, _ in CASES])
def test_bound_tells_right_from_wrong(shape, dtype, steps):
    S, Hkv, D, Hq = shape
    for T, older in steps:
        ref, out, vmax = answers(S, Hkv, D, Hq, dtype, T, older)
        r = {k: worst_ratio(v, ref, vmax, dtype) for k, v in out.items()}
        print(f"T {T} older {older}: " + "  ".join(f"{k} {v:.2f}" for k, v in r.items()))
        # rounding alone uses at most half of the 2u·A allowance
        assert r["right"] <= 0.5, (T, older, r)
        assert set(MUTANTS) <= set(r)
        for name in set(r) - {"right"}:
            assert not r[name] <= 1.0, (T, older, name, r)   # nan (a NaN row read) fails the check too


def test_onehot_map_tells_right_from_wrong():
    """The exact map of attn_checks.onehot_tail, emulated on the CPU in fp32 (sum of the visible one-hot rows over
    their number): the right visibility passes check_onehot; a row skipped, a row read twice and a causal
    limit one off for one query fail it, and so do a NaN and a value that should be an exact zero."""
    B, Hkv, G, D, T = 2, 2, 2, 128, 5
    counts = [131, 3]
    tk, tv = onehot_tail(B, max(counts) + 3, Hkv, D, torch.float32, counts, "cpu")
    vis = torch.stack([visible(T, n) for n in counts])                       # [B, T]

    def emulate(vis, times=None):
        out = torch.zeros(B, Hkv * G, T, D)
        for b in range(B):
            for t in range(T):
                v = int(vis[b, t])
                w = torch.ones(v) if times is None else times[b][:v]
                if w.sum() > 0:
                    row = (w[:, None] * tv[b, :v, :D]).sum(0) / w.sum()
                    out[b, :, t] = row
        return out

    assert (tk[0, :131] == 0).all() and torch.isnan(tk[0, 131:]).all() and torch.isnan(tv[1, 3:]).all()
    check_onehot(emulate(vis), vis[:, None, :])
    wrong = []
    for b, t, d in ((0, 2, 1), (0, 4, -1), (1, 0, 1), (1, 4, -1)):
        v = vis.clone()
        v[b, t] += d
        wrong.append(emulate(v))
    for b, u, k in ((0, 0, 0.0), (0, 130, 0.0), (0, 64, 2.0), (1, 2, 2.0)):        # a row skipped, a row twice
        times = [torch.ones(n) for n in counts]
        times[b][u] = k
        wrong.append(emulate(vis, times))
    nan = emulate(vis)
    nan[1, 3, 4, 5] = float("nan")
    tiny = emulate(vis)
    assert tiny[1, 0, 4, 3] == 0
    tiny[1, 0, 4, 3] = 1e-30
    for out in wrong + [nan, tiny]:
        with pytest.raises(AssertionError):
            check_onehot(out, vis[:, None, :])
