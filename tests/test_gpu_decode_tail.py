"""GPU: one decode step of attention over a packed layer followed by a dense tail of new tokens
(rtkv_decode_attention_packed_tail, decode_tail.hip) against a plain PyTorch fp32 reference over
cat(K'[:rows[b]], tail[:tail_rows[b]]) per batch row.

A decode step of the reference model does not compress: it concatenates the new token's K/V onto the
cache and attends over all of it (modified_llama.py:83-94, 152).  The kernel reads the packed rows
as rtkv_decode_attention_packed does and the tail rows as stored, one softmax over both.  The error
sources are those of tests/test_gpu_decode.py — fp32 summation order and the hardware exp2 — so the
tolerance is that file's: rtol = 2e-4, atol = 2e-5 · max(max|V'|, max|tail V|, 1).

Every unused tail row (capacity is always above the count) is filled with NaN: a finite output
within tolerance shows that nothing at or past the count is read.

Every layer keeps rows of all three precision classes (layer() asserts it), so each case decodes all
three field widths.  The field of a class is one bit wider than its bits where 2^bits − 1 is not a value
of the dtype (rtkv_field_width): bits (4, 8, 16) give the widths 4, 8 and 16 for float32, but 17 for
bfloat16 — outside the widths 2/4/8/16 the attention kernels take — and float16 with 16 bits is outside
what the quantizer accepts (tests/test_gpu_parity.py).  The 16-bit field of the two 16-bit dtypes is
that of a 15-bit class: (4, 8, 15)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import synth
from attn_checks import check_onehot, onehot_tail, visible

pytestmark = pytest.mark.gpu

TD = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
# Class thresholds that split these layers' tokens about evenly (30 / 33 / 37 % high / medium / low), and
# propagation ratios under which the budget runs out inside the lowest class: the high and the medium class are
# kept whole, the low class in part, so the kept index is not the identity.  The cost of a row is its width:
# with (2, 4, 8) a layer costs S · (high + medium / 2 + low / 4) ≈ 0.39 .. 0.59 · S, with (4, 8, 16) twice that.
COV = dict(alpha=0.8, beta=0.1, gamma=0.1, theta_h=0.5, theta_m=0.4)
RATIO = {620: 0.53, 800: 0.54, 650: 0.45}   # by S; every other S: 0.5.  (4, 8, 15) and (4, 8, 16): 1.0


def default_ratio(S, bits):
    return 1.0 if bits[2] >= 15 else RATIO.get(S, 0.5)
TAILS = (1, 3, 5, 257, 1500)   # one row; fewer than the 4 waves; 5; past one 64-row round; several tail splits


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    import rtkv
    rtkv.build()


def dev(stored: np.ndarray, dtype: str) -> torch.Tensor:
    if dtype == "float32":
        return torch.from_numpy(np.ascontiguousarray(stored, np.float32)).cuda()
    return torch.from_numpy(np.ascontiguousarray(stored, np.uint16).view(np.int16)).cuda().view(TD[dtype])


def rand(seed, shape, dtype, mul=1.0):
    return dev(synth.cast(synth.normal(seed, shape) * np.float32(mul), dtype), dtype)


_LAYERS = {}


def kept_classes(pk, b=0):
    """The precision class (0 low, 1 medium, 2 high) of each kept row of batch row b."""
    n = int(pk["rows"][b])
    return pk["labels"][b][pk["kept_index"][b, :n].long()].long()


def layer(B, S, Hkv, D, dtype, bits=(2, 4, 8), ratio=None):
    """(K', V', packed) of one compressed synthetic layer, computed once per shape and left unchanged.
    All three classes are among the kept rows of every batch row."""
    ratio = default_ratio(S, bits) if ratio is None else ratio
    key = (B, S, Hkv, D, dtype, bits, ratio)
    if key not in _LAYERS:
        import rtkv
        F = Hkv * D
        seed = S * 7 + Hkv
        K, V = synth.kv(seed, B, S, F, dtype)
        W = synth.attention_slice(seed, B, 8, S, rtkv.prompt_length(S), dtype)
        cfg = rtkv.CompressionConfig(num_hidden_layers=4, low_precision_bits=bits[0], medium_precision_bits=bits[1],
                                     high_precision_bits=bits[2], early_layer_ratio=ratio, middle_layer_ratio=ratio,
                                     later_layer_ratio=ratio, **COV)
        comp = rtkv.RealTimePrefillCompressor(cfg)
        ids = torch.zeros(B, S, dtype=torch.long, device="cuda")
        k2, v2, info = comp.compress_layer_kv_cache(dev(K, dtype), dev(V, dtype), dev(W, dtype), ids, 1)
        pk = info["packed"]
        for b in range(B):
            counts = torch.bincount(kept_classes(pk, b), minlength=3)
            assert (counts > 0).all() and int(pk["rows"][b]) < S, (key, b, counts.tolist())
        _LAYERS[key] = (k2, v2, pk)
    return _LAYERS[key]


def reference(k2, v2, rows, tk, tv, trows, q, Hkv, scale):
    """softmax(q·Xᵀ·scale)·Y in fp32 per batch row, X/Y = cat(K'/V'[:rows[b]], tail[:trows[b]])."""
    B, Hq, D = q.shape
    G = Hq // Hkv
    out = torch.zeros(B, Hq, D, dtype=torch.float32, device=q.device)
    for b in range(B):
        n, t = int(rows[b]), int(trows[b])
        if n + t == 0:
            continue
        Kf = torch.cat([k2[b, :n].float(), tk[b, :t].float()]).view(n + t, Hkv, D)
        Vf = torch.cat([v2[b, :n].float(), tv[b, :t].float()]).view(n + t, Hkv, D)
        qf = q[b].float().view(Hkv, G, D)
        s = torch.einsum("hgd,nhd->hgn", qf, Kf) * scale
        p = torch.softmax(s, dim=-1)
        out[b] = torch.einsum("hgn,nhd->hgd", p, Vf).reshape(Hq, D)
    return out


def make_tail(seed, B, T, F, dtype, spare=3, kmul=1.0):
    """Dense tail buffers [B, T + spare, F] with T rows in use and NaN in every unused row."""
    tk = rand(seed, (B, T + spare, F), dtype, kmul)
    tv = rand(seed + 1, (B, T + spare, F), dtype)
    tk[:, T:] = float("nan")
    tv[:, T:] = float("nan")
    return tk, tv


def check(out, ref, v2, tv, trows):
    assert torch.isfinite(out).all()
    tmax = max([tv[b, :int(t)].float().abs().max().item() for b, t in enumerate(trows) if int(t)] + [0.0])
    vmax = max(v2.float().abs().max().item() if v2.numel() else 0.0, tmax, 1.0)
    torch.testing.assert_close(out, ref, rtol=2e-4, atol=2e-5 * vmax)


SHAPES = [
    # S, Hkv, D, Hq            lane shape (chunks per lane, query heads per lane)
    (700, 4, 128, 4),        # F = 512, G = 1: 1 chunk, 1 head
    (900, 8, 128, 8),        # F = 1024, G = 1: 2 chunks
    (620, 4, 128, 8),        # G = 2: 2 heads
    (1000, 4, 128, 16),      # G = 4: 4 heads
    (800, 8, 64, 8),         # head_dim 64: lanes per head at run time
    (650, 2, 256, 16),       # head_dim 256, G = 8: 4 heads × 2 query-head groups
]
CASES = [(s, dt, (2, 4, 8)) for s in SHAPES[:3] for dt in ("float16", "bfloat16", "float32")] \
    + [(s, "float32", (4, 8, 16)) for s in SHAPES[:3]] \
    + [(s, dt, (4, 8, 15)) for s in SHAPES[:3] for dt in ("bfloat16", "float16")] \
    + [(s, "float16", (2, 4, 8)) for s in SHAPES[3:]]


@pytest.mark.parametrize("shape,dtype,bits", CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_packed_rows_then_tail(shape, dtype, bits):
    import rtkv
    S, Hkv, D, Hq = shape
    F = Hkv * D
    k2, v2, pk = layer(1, S, Hkv, D, dtype, bits)
    q = rand(S + 1, (1, Hq, D), dtype)
    for T in TAILS:
        tk, tv = make_tail(S + 10 * T, 1, T, F, dtype)
        tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([T]))
        out = rtkv.decode_attention(pk, q, Hkv, tail=tail)
        ref = reference(k2, v2, pk["rows"], tk, tv, [T], q, Hkv, 1.0 / D ** 0.5)
        check(out, ref, v2, tv, [T])
        assert torch.equal(rtkv.decode_attention(pk, q, Hkv, tail=tail), out)   # deterministic


@pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float32"])
def test_empty_tail_has_the_no_tail_bits(dtype):
    import rtkv
    S, Hkv, D, Hq = 900, 8, 128, 8
    k2, v2, pk = layer(1, S, Hkv, D, dtype)
    q = rand(5, (1, Hq, D), dtype)
    plain = rtkv.decode_attention(pk, q, Hkv)
    tk, tv = make_tail(6, 1, 0, Hkv * D, dtype, spare=8)
    tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert torch.equal(rtkv.decode_attention(pk, q, Hkv, tail=tail), plain)
    # existing callers still reach the old entry point: no append, no tail
    cache = rtkv.CompressedKVCache(1, S, D)
    cache.store_packed(0, pk)
    assert cache.tail_len(0) == 0 and torch.equal(cache.attend(0, q, Hkv), plain)
    # a freshly allocated tail (no token yet) changes nothing either
    assert torch.equal(rtkv.decode_attention(pk, q, Hkv, tail=rtkv.DecodeTail(1, Hkv * D, TD[dtype], "cuda", 4)), plain)


def test_batch_of_two_with_strided_tail():
    """Different kept counts per row, tail_rows = [0, 7], a batch stride larger than capacity · F."""
    import rtkv
    B, S, Hkv, D, Hq, dtype = 2, 800, 8, 128, 32, "float16"
    F = Hkv * D
    k2, v2, pk0 = layer(B, S, Hkv, D, dtype)
    pk = {k: v for k, v in pk0.items() if k != "_rows_dev"}
    pk["rows"] = [int(pk0["rows"][0]), int(pk0["rows"][1]) - 17]   # the first rows of row 1's kept list
    cap = 9
    big_k, big_v = make_tail(21, B, 0, F, dtype, spare=cap + 4)    # NaN everywhere
    tk, tv = big_k[:, :cap], big_v[:, :cap]
    tk[1, :7] = rand(22, (7, F), dtype)
    tv[1, :7] = rand(23, (7, F), dtype)
    assert tk.stride(0) > cap * F
    tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([0, 7]))
    q = rand(24, (B, Hq, D), dtype)
    out = rtkv.decode_attention(pk, q, Hkv, tail=tail)
    ref = reference(k2, v2, pk["rows"], tk, tv, [0, 7], q, Hkv, 1.0 / D ** 0.5)
    check(out, ref, v2, tv, [0, 7])
    # row 0 has no tail row: the bits of the packed-only step
    assert torch.equal(out[0], rtkv.decode_attention(pk, q, Hkv)[0])


def test_more_than_64_splits_in_one_list():
    """The packed and the tail splits are one list that the merge walks in 64 phases.  A packed row
    capacity of 2560 gives ceil(2560 / 64) = 40 packed splits and a tail capacity of 1920 gives
    ceil(1920 / 64) = 30 tail splits (both under the 1024-workgroup target: B·GS·HG = 1; the tuning
    knob RTKV_DECODE_WGS is taken as unset), 70 in all: merge phases 0 to 5 take two splits each
    (s and s + 64, the latter tail splits 24 to 29), phases 6 to 63 one.  The tail holds 100 rows, so
    a tail split owns ceil(100 / 30) = 4 rows: tail splits 0 to 24 have rows, 25 to 29 are empty
    (m = -inf) — and those are splits 65 to 69 of the list, the second ones of phases 1 to 5."""
    import rtkv
    import rtkv._lib as L
    S, Hkv, D, Hq, dtype = 700, 4, 128, 4, "float16"
    F, cap, tcap, T = Hkv * D, 2560, 1920, 100
    k2, v2, pk0 = layer(1, S, Hkv, D, dtype)
    n0 = pk0["kept_index"].shape[1]
    assert 0 < n0 <= cap
    pk = {k: v for k, v in pk0.items() if k != "_rows_dev"}
    for name in ("row_offset", "scale_zp", "kept_index"):       # the same rows in a layer of capacity 2560
        t = pk0[name]
        pk[name] = torch.cat([t, torch.zeros(1, cap - n0, *t.shape[2:], dtype=t.dtype, device=t.device)], 1)
    # 40 and 30 splits of (2·Hkv + F) floats, as rtkv_decode_tail_workspace_size lays them out
    part = (2 * Hkv + F) * 4
    assert L.lib().rtkv_decode_tail_workspace_size(1, Hq, Hkv, D, cap, tcap) \
        == (40 * part + 256 + 255) // 256 * 256 + 30 * part + 256
    q = rand(71, (1, Hq, D), dtype)
    tk, tv = make_tail(72, 1, T, F, dtype, spare=tcap - T)
    out = rtkv.decode_attention(pk, q, Hkv, tail=rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([T])))
    ref = reference(k2, v2, pk["rows"], tk, tv, [T], q, Hkv, 1.0 / D ** 0.5)
    check(out, ref, v2, tv, [T])
    # no tail row: every tail split is empty, the bits of the packed-only step
    none = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([0]))
    assert torch.equal(rtkv.decode_attention(pk, q, Hkv, tail=none), rtkv.decode_attention(pk, q, Hkv))


def empty_packed(B, F, dtype):
    z = lambda *s, dt: torch.zeros(*s, dtype=dt, device="cuda")  # noqa: E731
    return {"codes_k": z(0, dt=torch.uint8), "codes_v": z(0, dt=torch.uint8), "row_offset": z(B, 0, dt=torch.int64),
            "scale_zp": z(B, 0, 4, dt=torch.float32), "kept_index": z(B, 0, dt=torch.int32),
            "labels": z(B, 8, dt=torch.uint8), "rows": [0] * B, "bits": (2, 4, 8), "dtype": TD[dtype], "feature_dim": F}


@pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float32"])
def test_tail_only(dtype):
    """No packed row (rows = [0]) and no packed capacity at all (S' == 0 tensors): attention over
    the tail alone; neither with a tail row: zeros."""
    import rtkv
    S, Hkv, D, Hq = 620, 4, 128, 8
    F = Hkv * D
    k2, v2, pk0 = layer(1, S, Hkv, D, dtype)
    none = {k: v for k, v in pk0.items() if k != "_rows_dev"}
    none["rows"] = [0]
    q = rand(31, (1, Hq, D), dtype)
    for T in (1, 70):
        tk, tv = make_tail(32 + T, 1, T, F, dtype)
        tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([T]))
        ref = reference(k2[:, :0], v2[:, :0], [0], tk, tv, [T], q, Hkv, 1.0 / D ** 0.5)
        for p in (none, empty_packed(1, F, dtype)):
            check(rtkv.decode_attention(p, q, Hkv, tail=tail), ref, v2[:, :0], tv, [T])
    tk, tv = make_tail(40, 1, 0, F, dtype, spare=5)
    tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([0]))
    for p in (none, empty_packed(1, F, dtype)):
        assert torch.count_nonzero(rtkv.decode_attention(p, q, Hkv, tail=tail)) == 0


@pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float32"])
def test_dominance_both_ways(dtype):
    """The running maximum across the packed/tail merge.  A tail key equal to q for one query head
    (|q|²/√D ≈ 16·√D, far above q·k of any other row) puts that head's whole weight on its tail row;
    a tail of tiny keys (scores ≈ 0, below the packed rows' maximum) only mixes in per the reference."""
    import rtkv
    S, Hkv, D, Hq = 620, 4, 128, 8
    F, G = Hkv * D, Hq // Hkv
    k2, v2, pk = layer(1, S, Hkv, D, dtype)
    q = rand(41, (1, Hq, D), dtype, mul=4.0)
    T, t_hit, hq = 5, 3, 5
    tk, tv = make_tail(42, 1, T, F, dtype)
    h = hq // G
    tk[0, t_hit, h * D:(h + 1) * D] = q[0, hq]
    tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([T]))
    out = rtkv.decode_attention(pk, q, Hkv, tail=tail)
    ref = reference(k2, v2, pk["rows"], tk, tv, [T], q, Hkv, 1.0 / D ** 0.5)
    check(out, ref, v2, tv, [T])
    vmax = max(v2.float().abs().max().item(), tv[:, :T].float().abs().max().item(), 1.0)
    torch.testing.assert_close(out[0, hq], tv[0, t_hit, h * D:(h + 1) * D].float(), rtol=2e-4, atol=2e-5 * vmax)
    # the other way: tiny tail keys
    tk, tv = make_tail(44, 1, 70, F, dtype, kmul=1e-3)
    tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([70]))
    out = rtkv.decode_attention(pk, q, Hkv, tail=tail)
    ref = reference(k2, v2, pk["rows"], tk, tv, [70], q, Hkv, 1.0 / D ** 0.5)
    check(out, ref, v2, tv, [70])


def lead(X, q, D):
    """(argmax, its lead in nats over every other row) of the scores q·Xᵀ/√D; X [N, D], q [D]."""
    sc = X.double() @ q.double() / math.sqrt(D)
    r = int(sc.argmax())
    return r, (sc[r] - torch.cat([sc[:r], sc[r + 1:]]).max()).item() if sc.numel() > 1 else float("inf")


def aimed_query(kh, r, D, dtype):
    """A multiple of row r of kh [n, D] under which that row's score leads every other row of kh by 60 nats
    (before the rounding to the dtype): c · kh[r], c = 60·√D / (|kh[r]|² − max_j kh[j]·kh[r])."""
    dots = kh.double() @ kh[r].double()
    gap = (dots[r] - torch.cat([dots[:r], dots[r + 1:]]).max()).item()
    assert gap > 0, (r, gap)
    return (kh[r].double() * (60.0 * math.sqrt(D) / gap)).to(TD[dtype])


def single_rows(pk, b=0):
    """The kept rows a single-row test aims at: the first row of each class, the last kept row (its width
    comes from its class label, not from its byte span) and, where the layer has more than one split, the
    first row of the second split of decode.hip (ceil(capacity / 64) splits) and of extend.hip (ceil(capacity
    / 128)); both kernels give split s the rows [s · per, (s + 1) · per), per = ceil(rows / splits)."""
    n, cap = int(pk["rows"][b]), pk["kept_index"].shape[1]
    cls = kept_classes(pk, b)
    rows = {f"first row of class {c}": int((cls == c).nonzero()[0]) for c in range(3)}
    rows["last kept row"] = n - 1
    for name, per_split in (("decode split 1", 64), ("extend split 1", 128)):
        splits = -(-cap // per_split)
        if splits > 1 and -(-n // splits) < n:
            rows[name] = -(-n // splits)
    return rows


def swapped(pk):
    """The layer with K and V exchanged (codes and scale / zero-point columns): its attention output is a
    row of K', so the kernel's decode of the K codes is compared element for element as well."""
    sw = {k: v for k, v in pk.items() if k != "_rows_dev"}
    sw["codes_k"], sw["codes_v"] = pk["codes_v"], pk["codes_k"]
    sw["scale_zp"] = pk["scale_zp"][..., [2, 3, 0, 1]].contiguous()
    return sw


SINGLE = [("float16", (2, 4, 8)), ("bfloat16", (2, 4, 8)), ("float16", (4, 8, 15)), ("bfloat16", (4, 8, 15)),
          ("float32", (2, 4, 8)), ("float32", (4, 8, 16))]
# Why rtol = 1e-5 and atol = 1e-8·vmax in the single-row tests: the test asserts that the row leads every
# other visible row by more than 30 nats, so the others weigh less than N·e⁻³⁰ < 2100 · 9.4e-14 = 2e-10 together
# and move the output by less than 4e-10·vmax; the row's own weight is exp2(0) = 1 (the running maximum is its
# score), so what is left is a few fp32 roundings (1.2e-7 relative).  One ulp of a float16 value is 4.9e-4 of
# it, of a bfloat16 value 3.9e-3: a dequantization that is one ulp off fails.
SINGLE_RTOL, SINGLE_ATOL = 1e-5, 1e-8


@pytest.mark.parametrize("dtype,bits", SINGLE, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_one_packed_row_takes_the_whole_weight(dtype, bits):
    """q of one query head a multiple of K'[r] of its kv head: the head's output is V'[r], for one row of
    each class (each field width), the last kept row and the first row of a later split — and the same with
    K and V exchanged, where the output is K'[r]."""
    import rtkv
    S, Hkv, D, Hq = 620, 4, 128, 8
    F, G, T, hq = Hkv * D, Hq // Hkv, 5, 5
    h = hq // G
    k2, v2, pk = layer(1, S, Hkv, D, dtype, bits)
    n = int(pk["rows"][0])
    tk, tv = make_tail(202, 1, T, F, dtype)
    tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([T]))
    for p, X, Y in ((pk, k2, v2), (swapped(pk), v2, k2)):
        Xh = X[0, :n, h * D:(h + 1) * D]
        vmax = max(Y[0, :n].float().abs().max().item(), tv[:, :T].float().abs().max().item(), 1.0)
        for name, r in single_rows(pk).items():
            q = rand(203, (1, Hq, D), dtype)
            q[0, hq] = aimed_query(Xh, r, D, dtype)
            top, by = lead(torch.cat([Xh, tk[0, :T, h * D:(h + 1) * D]]), q[0, hq], D)
            assert top == r and by > 30, (name, r, top, by)
            out = rtkv.decode_attention(p, q, Hkv, tail=tail)
            row = Y[0, r, h * D:(h + 1) * D].float()
            err = (out[0, hq] - row).abs().max().item()
            print(f"{name} (row {r} of {n}, class {int(kept_classes(pk)[r])}): lead {by:.1f} nats, "
                  f"max |out - row| {err:.2e}")
            torch.testing.assert_close(out[0, hq], row, rtol=SINGLE_RTOL, atol=SINGLE_ATOL * vmax,
                                       msg=lambda m: f"{name}: {m}")


@pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float32"])
def test_onehot_tail_map(dtype):
    """Zero keys and one-hot values (attn_checks.onehot_tail) and no packed row: every weight is exactly 1,
    so out[b, hq, c] = #{u < n : u mod D = c} / n with no tolerance — a tail row skipped or read twice shows
    in its channel.  Counts around the 64-row round of the four waves and with several tail splits."""
    import rtkv
    Hkv, D, Hq = 4, 128, 8
    k2, v2, pk0 = layer(1, 620, Hkv, D, dtype)
    none = {k: v for k, v in pk0.items() if k != "_rows_dev"}
    none["rows"] = [0]
    q = rand(211, (1, Hq, D), dtype)
    for n in (1, 3, 63, 64, 65, 257, 1500):
        tk, tv = onehot_tail(1, n + 3, Hkv, D, TD[dtype], [n], "cuda")
        tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([n]))
        for name, p in (("rows = [0]", none), ("no packed capacity", empty_packed(1, Hkv * D, dtype))):
            check_onehot(rtkv.decode_attention(p, q, Hkv, tail=tail), torch.tensor([[n]]), f"{dtype} n = {n}, {name}")


def test_17_bit_fields_are_refused():
    """bfloat16 with a 16-bit class packs 17-bit fields (rtkv_field_width): both attention entry points refuse
    the layer by name instead of reading it with another width."""
    import rtkv
    S, Hkv, D, Hq, dtype = 620, 4, 128, 8, "bfloat16"
    k2, v2, pk = layer(1, S, Hkv, D, dtype, (4, 8, 16))
    tk, tv = make_tail(221, 1, 4, Hkv * D, dtype)
    tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([4]))
    for call in (lambda: rtkv.decode_attention(pk, rand(222, (1, Hq, D), dtype), Hkv),
                 lambda: rtkv.decode_attention(pk, rand(222, (1, Hq, D), dtype), Hkv, tail=tail),
                 lambda: rtkv.extend_attention(pk, rand(223, (1, Hq, 3, D), dtype), Hkv, tail)):
        with pytest.raises(RuntimeError, match="field widths 2/4/8/16 only"):
            call()
    torch.cuda.synchronize()


def test_count_above_capacity_is_clamped():
    import rtkv
    S, Hkv, D, Hq, dtype = 700, 4, 128, 4, "float16"
    k2, v2, pk = layer(1, S, Hkv, D, dtype)
    cap = 6
    tk, tv = make_tail(51, 1, cap, Hkv * D, dtype, spare=0)
    q = rand(52, (1, Hq, D), dtype)
    full = rtkv.decode_attention(pk, q, Hkv, tail=rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([cap])))
    over = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([cap + 1000], device="cuda"))
    assert torch.equal(rtkv.decode_attention(pk, q, Hkv, tail=over), full)
    neg = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([-3], device="cuda"))
    assert torch.equal(rtkv.decode_attention(pk, q, Hkv, tail=neg), rtkv.decode_attention(pk, q, Hkv))


def test_rejected_input():
    import rtkv
    import rtkv._lib as L
    S, Hkv, D, Hq, dtype = 700, 4, 128, 4, "float16"
    F = Hkv * D
    k2, v2, pk = layer(1, S, Hkv, D, dtype)
    q = rand(61, (1, Hq, D), dtype)
    tk, tv = make_tail(62, 1, 2, F, dtype)
    good = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([2]))
    with pytest.raises(ValueError):
        rtkv.decode_attention(pk, q.float(), Hkv, tail=good)                     # q of another dtype
    with pytest.raises(ValueError):
        rtkv.decode_attention(pk, q, Hkv, tail=rtkv.DecodeTail(1, F, torch.bfloat16, "cuda", 4))
    wide = rand(63, (1, 5, F + 4), dtype)
    with pytest.raises(ValueError):
        rtkv.DecodeTail.from_tensors(wide[:, :, :F], wide[:, :, :F], torch.tensor([2]))   # misaligned rows
    # the same buffers handed to the library without the Python check: refused there, nothing launched
    raw = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([2]))
    raw.k = raw.v = wide[:, :, :F]
    with pytest.raises(RuntimeError, match="decode"):
        rtkv.decode_attention(pk, q, Hkv, tail=raw)
    raw.k = raw.v = wide.reshape(-1)[4:4 + 5 * F].view(1, 5, F)                  # base 8 bytes off
    with pytest.raises(RuntimeError, match="decode"):
        rtkv.decode_attention(pk, q, Hkv, tail=raw)
    # the C ABI's own argument checks (tail-only call: the packed pointers may be null)
    out = torch.zeros(1, Hq, D, device="cuda")
    ws_bytes = L.lib().rtkv_decode_tail_workspace_size(1, Hq, Hkv, D, 0, 5)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    rows_dev = torch.tensor([2], device="cuda")

    def call(t, nbytes):
        return L.lib().rtkv_decode_attention_packed_tail(0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, Hkv, D, L.F16, None,
                                                         q.data_ptr(), Hq, 0.1, ctypes.byref(t), out.data_ptr(),
                                                         ws.data_ptr(), nbytes, L.stream_ptr(q.device))
    ok = L.DenseTail(tk.data_ptr(), tv.data_ptr(), rows_dev.data_ptr(), 5, tk.stride(0), tk.stride(1))
    assert call(ok, ws_bytes) == 0
    for bad, nbytes in ((L.DenseTail(tk.data_ptr(), tv.data_ptr(), rows_dev.data_ptr(), -1, tk.stride(0), F), ws_bytes),
                        (L.DenseTail(tk.data_ptr(), tv.data_ptr(), 0, 5, tk.stride(0), F), ws_bytes),
                        (L.DenseTail(tk.data_ptr(), tv.data_ptr(), rows_dev.data_ptr(), 5, tk.stride(0), F + 4), ws_bytes),
                        (ok, ws_bytes - 1024)):
        assert call(bad, nbytes) == -1                                           # RTKV_ERR_INVALID
        assert "decode: " in L.lib().rtkv_last_error().decode()
    torch.cuda.synchronize()


def test_generation_loop():
    """store_packed, then 6 decode steps through CompressedDecodeAttention with a tail that starts
    at 4 rows and grows mid-loop; each step against torch over cat(K', tokens so far)."""
    import rtkv
    B, S, Hkv, D, Hq, dtype = 1, 512, 8, 128, 32, "float16"
    F = Hkv * D
    k2, v2, pk = layer(B, S, Hkv, D, dtype)
    cache = rtkv.CompressedKVCache(B, S, D, tail_capacity=4)
    cache.store_packed(2, pk)
    att = rtkv.CompressedDecodeAttention(cache, Hq, Hkv, D, 2)
    ks, vs = [], []
    for step in range(6):
        q = rand(70 + step, (B, Hq, 1, D), dtype)
        k = rand(80 + step, (B, Hkv, 1, D), dtype)
        v = rand(90 + step, (B, Hkv, 1, D), dtype)
        out = att(q, k, v)
        assert out.shape == (B, 1, Hq * D) and out.dtype == TD[dtype]
        assert cache.tail_len(2) == step + 1
        ks.append(k.transpose(1, 2).reshape(B, 1, F))
        vs.append(v.transpose(1, 2).reshape(B, 1, F))
        tk, tv = torch.cat(ks, 1), torch.cat(vs, 1)
        ref = reference(k2, v2, pk["rows"], tk, tv, [step + 1], q[:, :, 0], Hkv, 1.0 / D ** 0.5)
        # the module returns the fp32 result rounded to the query dtype
        vmax = max(v2.float().abs().max().item(), tv.float().abs().max().item(), 1.0)
        full = cache.attend(2, q[:, :, 0], Hkv)
        torch.testing.assert_close(full, ref, rtol=2e-4, atol=2e-5 * vmax)
        assert torch.equal(out, full.to(TD[dtype]).reshape(B, 1, Hq * D))
    assert cache.tails[2].capacity == 8
    with pytest.raises(ValueError):
        att(q, k, v, attention_mask=torch.zeros(B, 1, 1, 1, device="cuda"))
    cache.store_packed(2, pk)
    assert cache.tail_len(2) == 0
    assert torch.equal(cache.attend(2, q[:, :, 0], Hkv), rtkv.decode_attention(pk, q[:, :, 0], Hkv))
