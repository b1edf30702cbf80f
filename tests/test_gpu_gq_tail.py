"""GPU: generation on the group-quantized cache — one decode step over a layer in the rtkv-gq/1 format
followed by a dense tail of new tokens (rtkv_gq_decode_attention_tail, csrc/gq_decode.hip), and the Python
chain above it (GroupQuantKVCache.attend(tail=), CompressedKVCache.store_group_quant / append / attend /
attend_chunk, CompressedDecodeAttention).

Reference: torch fp32 softmax over cat(cache.dequantize(), tail rows in use), repeat_interleave for GQA.  The
kernel decodes K'/V' to exactly the values rtkv_gq_unpack writes (what dequantize() returns) and its
attention arithmetic is the decode family's (fp32 dot products and sums, hardware exp2), so the tolerance
is that family's (tests/test_gpu_decode_tail.py): rtol = 2e-4, atol = 2e-5 · max(max|V'|, max|tail V|, 1).

Layers come from the drop-in with group_quant=; per-channel outliers are injected in K AND V, two of
them inside one 8-element chunk (channels 3 and 5), and each test asserts that both tensors' outlier
lists hold channels, so a missing raw-value patch cannot pass.  Every unused tail row is NaN."""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

import synth
from attn_checks import check_onehot, onehot_tail

pytestmark = pytest.mark.gpu

TD = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
K_OUT = (3, 5, 77, 100)     # outlier channels of every head of K (3 and 5 share a chunk)
V_OUT = (10, 12, 64, 127)   # and of V (10 and 12 share a chunk)
GAIN = 25.0


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
# Propagation ratios that leave all three classes among the kept rows (the 2-bit class is dropped first):
# 0.9 keeps every row of these layers; at S = 1300, 0.83 drops most of the 2-bit rows but not all, so the
# kept index is not the identity there.
RATIO = {1300: 0.83}


def layer(dtype, S, H, n_out):
    """One compressed layer with the extension on, computed once per shape and left unchanged:
    (cache, K', V', Kd, Vd) — K'/V' = cache.dequantize() [rows, F], Kd/Vd the layer's device inputs."""
    ratio = RATIO.get(S, 0.9)
    key = (dtype, S, H, n_out, ratio)
    if key not in _LAYERS:
        import rtkv
        F = H * 128
        seed = 900 + S + H
        K, V = synth.kv(seed, 1, S, F, "float32")
        K, V = K.copy(), V.copy()
        for h in range(H):
            for c in K_OUT:
                K[..., h * 128 + c] *= GAIN
            for c in V_OUT:
                V[..., h * 128 + c] *= GAIN
        W = synth.attention_slice(seed, 1, 8, S, min(S // 5, 128), "float32")
        cfg = rtkv.CompressionConfig(alpha=0.8, beta=0.1, gamma=0.1, theta_h=0.4, theta_m=0.25, num_hidden_layers=4,
                                     high_precision_bits=8, medium_precision_bits=4, low_precision_bits=2,
                                     early_layer_ratio=ratio, middle_layer_ratio=ratio, later_layer_ratio=ratio)
        gqc = rtkv.GroupQuantConfig(n_outlier=n_out, n_vote=4, vote_stride=3, min_votes_pm=250)
        comp = rtkv.RealTimePrefillCompressor(cfg, group_quant=gqc)
        Kd, Vd = dev(synth.cast(K, dtype), dtype), dev(synth.cast(V, dtype), dtype)
        ids = torch.zeros(1, S, dtype=torch.long, device="cuda")
        _, _, info = comp.compress_layer_kv_cache(Kd, Vd, dev(synth.cast(W, dtype), dtype), ids, 1)
        c = info["group_quant"]
        kq, vq = c.dequantize()
        torch.cuda.synchronize()
        # all three classes (2, 4 and 8-bit rows) are among the kept rows
        kept = c.kept_index[:c.rows].long()
        assert torch.unique(c.labels[kept]).numel() == 3, torch.bincount(c.labels[kept].long())
        _LAYERS[key] = (c, kq[0], vq[0], Kd, Vd)
    c = _LAYERS[key][0]
    if n_out:  # both tensors have outlier channels: the raw-value patch is exercised for K and for V
        oi = c.outlier_idx.cpu()
        assert (oi[0] >= 0).any() and (oi[1] >= 0).any(), oi
    return _LAYERS[key]


def reference(kq, vq, n, tk, tv, t, q, H, scale=1.0 / math.sqrt(128)):
    """softmax(q·Xᵀ·scale)·Y in fp32, X/Y = cat(K'/V'[:n], tail[:t]); q [1, Hq, 128] → [1, Hq, 128]."""
    Hq = q.shape[1]
    G = Hq // H
    out = torch.zeros(1, Hq, 128, dtype=torch.float32, device=q.device)
    if n + t == 0:
        return out
    Kf = torch.cat([kq[:n].float(), tk[0, :t].float()]).view(n + t, H, 128).repeat_interleave(G, dim=1)
    Vf = torch.cat([vq[:n].float(), tv[0, :t].float()]).view(n + t, H, 128).repeat_interleave(G, dim=1)
    s = torch.einsum("hd,nhd->hn", q[0].float(), Kf) * scale
    out[0] = torch.einsum("hn,nhd->hd", torch.softmax(s, dim=-1), Vf)
    return out


def make_tail(seed, T, F, dtype, spare=3, kmul=1.0):
    """Dense tail buffers [1, T + spare, F] with T rows in use and NaN in every unused row."""
    tk = rand(seed, (1, T + spare, F), dtype, kmul)
    tv = rand(seed + 1, (1, T + spare, F), dtype)
    tk[:, T:] = float("nan")
    tv[:, T:] = float("nan")
    return tk, tv


def check(out, ref, vq, tv, t):
    assert torch.isfinite(out).all()
    tmax = tv[0, :t].float().abs().max().item() if t else 0.0
    vmax = max(vq.float().abs().max().item() if vq.numel() else 0.0, tmax, 1.0)
    err = (out - ref).abs().max().item()
    print(f"max |out - ref| = {err:.3g}, atol = {2e-5 * vmax:.3g}, max |ref| = {ref.abs().max().item():.3g}")
    torch.testing.assert_close(out, ref, rtol=2e-4, atol=2e-5 * vmax)


# (H, Hq): one chunk column; two; three head groups; G = 2; G = 4 — and the S of each
SHAPES = [(4, 4, 1500), (8, 8, 2000), (12, 12, 1100), (4, 8, 1300), (4, 16, 1000)]
N_OUT = (0, 4, 16)
TAILS = (1, 70, 300)
# 7 cases per dtype: every shape, every n_outlier and every tail length appears with every dtype
CASES = [(dt, SHAPES[i % 5], N_OUT[(i + d) % 3], TAILS[(i + 2 * d) % 3])
         for d, dt in enumerate(("float16", "bfloat16", "float32")) for i in range(7)]


@pytest.mark.parametrize("dtype,shape,n_out,T", CASES,
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_gq_rows_then_tail(dtype, shape, n_out, T):
    import rtkv
    H, Hq, S = shape
    c, kq, vq, _, _ = layer(dtype, S, H, n_out)
    q = rand(S + Hq, (1, Hq, 128), dtype)
    tk, tv = make_tail(S + 10 * T, T, H * 128, dtype)
    tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([T]))
    out = c.attend(q, tail=tail)
    check(out, reference(kq, vq, c.rows, tk, tv, T, q, H), vq, tv, T)
    assert torch.equal(c.attend(q, tail=tail), out)   # deterministic


@pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float32"])
def test_empty_tail(dtype):
    """Capacity 16, count 0: the torch reference over the gq rows, and the old kernel at its test's 2e-3."""
    import rtkv
    H, Hq, S = 8, 8, 2000
    c, kq, vq, _, _ = layer(dtype, S, H, 4)
    q = rand(5, (1, Hq, 128), dtype)
    tk, tv = make_tail(6, 0, H * 128, dtype, spare=16)
    tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.zeros(1, dtype=torch.int64, device="cuda"))
    out = c.attend(q, tail=tail)
    ref = reference(kq, vq, c.rows, tk, tv, 0, q, H)
    check(out, ref, vq, tv, 0)
    old = c.attend(q)
    assert (out - old).abs().max().item() <= 2e-3 * max(1.0, ref.abs().max().item())


def with_stats_kept(c, kept):
    """A shallow copy of the cache whose device statistics say `kept` rows."""
    import rtkv._lib as L
    c2 = copy.copy(c)
    c2.stats = c.stats.clone()
    at = ctypes.sizeof(L.LayerStatsHeader) + L.BatchStats.kept.offset
    c2.stats.view(torch.uint8)[at:at + 8] = torch.tensor([kept], dtype=torch.int64).view(torch.uint8).cuda()
    return c2


def test_device_side_counts():
    import rtkv
    dtype, H, Hq, S = "float16", 4, 8, 1300
    F = H * 128
    c, kq, vq, _, _ = layer(dtype, S, H, 4)
    q = rand(31, (1, Hq, 128), dtype)
    T = 7
    tk, tv = make_tail(32, T, F, dtype)
    # the kept count zeroed on the device: the tail alone
    none = with_stats_kept(c, 0)
    out = none.attend(q, tail=rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([T])))
    check(out, reference(kq, vq, 0, tk, tv, T, q, H), vq[:0], tv, T)
    # both counts 0: zeros
    zero = rtkv.DecodeTail.from_tensors(tk, tv, torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert torch.count_nonzero(none.attend(q, tail=zero)) == 0
    # a tail count above capacity is clamped (and a negative one to 0)
    fk, fv = make_tail(33, 6, F, dtype, spare=0)
    full = c.attend(q, tail=rtkv.DecodeTail.from_tensors(fk, fv, torch.tensor([6])))
    over = rtkv.DecodeTail.from_tensors(fk, fv, torch.tensor([6 + 1000], device="cuda"))
    assert torch.equal(c.attend(q, tail=over), full)
    check(full, reference(kq, vq, c.rows, fk, fv, 6, q, H), vq, fv, 6)
    neg = rtkv.DecodeTail.from_tensors(fk, fv, torch.tensor([-3], device="cuda"))
    assert torch.equal(c.attend(q, tail=neg), c.attend(q, tail=zero))
    # a kept count above the row capacity is clamped to it
    assert torch.equal(with_stats_kept(c, c.rows + 1000).attend(q, tail=over), full)
    # NaN tail rows at or past the count (make_tail), 0xFF code bytes past the last kept row
    pad = copy.copy(c)
    ff = torch.full((4096,), 0xFF, dtype=torch.uint8, device="cuda")
    pad.codes_k, pad.codes_v = torch.cat([c.codes_k, ff]), torch.cat([c.codes_v, ff])
    tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([T]))
    out = pad.attend(q, tail=tail)
    check(out, reference(kq, vq, c.rows, tk, tv, T, q, H), vq, tv, T)
    assert torch.equal(out, c.attend(q, tail=tail))


@pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float32"])
def test_onehot_tail_map(dtype):
    """The device kept count set to 0, zero tail keys and one-hot tail values (attn_checks.onehot_tail): every
    weight is exactly 1, so out[0, hq, c] = #{u < n : u mod 128 = c} / n with no tolerance — a tail row skipped
    or read twice shows in its channel.  Counts around the 64-row round of the four waves and with several
    tail splits; unused rows are NaN."""
    import rtkv
    H, Hq, S = 4, 8, 1300
    c, _, _, _, _ = layer(dtype, S, H, 4)
    none = with_stats_kept(c, 0)
    q = rand(35, (1, Hq, 128), dtype)
    for n in (1, 3, 63, 64, 65, 257, 1500):
        tk, tv = onehot_tail(1, n + 3, H, 128, TD[dtype], [n], "cuda")
        out = none.attend(q, tail=rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([n])))
        check_onehot(out, torch.tensor([[n]]), f"{dtype} n = {n}")


def scores(kq, n, tk, t, q, H, hq):
    """exp-domain scores of query head hq over cat(K'[:n], tail[:t]) (natural log units)."""
    G = q.shape[1] // H
    h = hq // G
    X = torch.cat([kq[:n].float(), tk[0, :t].float()])[:, h * 128:(h + 1) * 128]
    return X @ q[0, hq].float() / math.sqrt(128)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float32"])
def test_dominance_both_ways(dtype):
    """The running maximum across the gq/tail merge.  One head's whole weight on one tail row (a tail key
    equal to q); then on one gq row (q a multiple of that row's K', the row of the largest norm, so by
    Cauchy-Schwarz its score is the largest): the output is that row of dequantize()'s V', outlier channels
    included."""
    import rtkv
    H, Hq, S = 4, 8, 1300
    F, G = H * 128, 2
    c, kq, vq, _, _ = layer(dtype, S, H, 4)
    n = c.rows
    q = rand(41, (1, Hq, 128), dtype, mul=4.0)
    T, t_hit, hq = 5, 3, 5
    h = hq // G
    tk, tv = make_tail(42, T, F, dtype)
    tk[0, t_hit, h * 128:(h + 1) * 128] = q[0, hq]
    s = scores(kq, n, tk, T, q, H, hq)
    assert s.argmax().item() == n + t_hit and (s[n + t_hit] - torch.cat([s[:n + t_hit], s[n + t_hit + 1:]]).max()) > 30
    out = c.attend(q, tail=rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([T])))
    check(out, reference(kq, vq, n, tk, tv, T, q, H), vq, tv, T)
    vmax = max(vq.float().abs().max().item(), tv[:, :T].float().abs().max().item(), 1.0)
    torch.testing.assert_close(out[0, hq], tv[0, t_hit, h * 128:(h + 1) * 128].float(), rtol=2e-4, atol=2e-5 * vmax)
    # the other way: one gq row
    kh = kq[:n, h * 128:(h + 1) * 128].float()
    r = kh.norm(dim=1).argmax().item()
    dots = kh @ kh[r]
    gap = (dots[r] - torch.cat([dots[:r], dots[r + 1:]]).max()).item()
    assert gap > 0
    q2 = q.clone()
    q2[0, hq] = (kh[r] * (60.0 * math.sqrt(128) / gap)).to(TD[dtype])
    tk, tv = make_tail(44, 70, F, dtype)
    s = scores(kq, n, tk, 70, q2, H, hq)
    assert s.argmax().item() == r and (s[r] - torch.cat([s[:r], s[r + 1:]]).max()) > 30
    out = c.attend(q2, tail=rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([70])))
    check(out, reference(kq, vq, n, tk, tv, 70, q2, H), vq, tv, 70)
    row = vq[r, h * 128:(h + 1) * 128].float()
    torch.testing.assert_close(out[0, hq], row, rtol=2e-4, atol=2e-5 * vmax)
    oi = c.outlier_idx[1, h].cpu()
    assert (oi >= 0).any()   # the row holds raw outlier values of V


def test_more_than_64_splits_in_one_list():
    """The gq and the tail splits are one list that the merge walks in 64 phases.  A row capacity of 2560
    gives 40 gq splits and a tail capacity of 1920 gives 30 tail splits (B·GS·HG = 1, under the
    1024-workgroup target; RTKV_DECODE_WGS taken as unset), 70 in all.  With every kept row, each gq split
    has rows; with the device count set to 100, a gq split owns ceil(100 / 40) = 3 rows and splits 34 to 39
    are empty.  The tail holds 100 rows: tail splits 0 to 24 have 4 rows, 25 to 29 are empty (m = -inf) —
    splits 65 to 69 of the list, the second ones of merge phases 1 to 5."""
    import rtkv
    import rtkv._lib as L
    dtype, H, Hq, S = "float16", 4, 4, 2500
    F, cap, tcap, T = H * 128, 2560, 1920, 100
    c, kq, vq, _, _ = layer(dtype, S, H, 4)
    n0 = c.rows
    assert 100 < n0 <= cap
    part = (2 * H + F) * 4
    assert L.lib().rtkv_gq_decode_tail_workspace_size(Hq, H, cap, tcap) == 70 * part + 256
    big = copy.copy(c)   # the same rows in a layer of capacity 2560 (the device count stops at the n0 rows held)
    big.rows = cap
    for name in ("meta", "raw"):
        t = getattr(c, name)
        setattr(big, name, torch.cat([t, torch.zeros(cap - n0, *t.shape[1:], dtype=t.dtype, device=t.device)]))
    q = rand(71, (1, Hq, 128), dtype)
    tk, tv = make_tail(72, T, F, dtype, spare=tcap - T)
    tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([T]))
    check(big.attend(q, tail=tail), reference(kq, vq, n0, tk, tv, T, q, H), vq, tv, T)
    few = with_stats_kept(big, 100)
    check(few.attend(q, tail=tail), reference(kq, vq, 100, tk, tv, T, q, H), vq, tv, T)


def test_generation_loop():
    """store_group_quant, then 6 decode steps through CompressedDecodeAttention with a tail that starts at 2
    rows and doubles twice; each step against torch over cat(K', tokens so far)."""
    import rtkv
    dtype, H, Hq, S = "float16", 8, 32, 2000
    F = H * 128
    c, kq, vq, _, _ = layer(dtype, S, H, 4)
    cache = rtkv.CompressedKVCache(1, S, 128, tail_capacity=2)
    cache.store_group_quant(2, c)
    att = rtkv.CompressedDecodeAttention(cache, Hq, H, 128, 2)
    ks, vs = [], []
    for step in range(6):
        q = rand(70 + step, (1, Hq, 1, 128), dtype)
        k = rand(80 + step, (1, H, 1, 128), dtype)
        v = rand(90 + step, (1, H, 1, 128), dtype)
        out = att(q, k, v)
        assert out.shape == (1, 1, Hq * 128) and out.dtype == TD[dtype]
        assert cache.tail_len(2) == step + 1
        ks.append(k.transpose(1, 2).reshape(1, 1, F))
        vs.append(v.transpose(1, 2).reshape(1, 1, F))
        tk, tv = torch.cat(ks, 1), torch.cat(vs, 1)
        ref = reference(kq, vq, c.rows, tk, tv, step + 1, q[:, :, 0], H)
        full = cache.attend(2, q[:, :, 0], H)
        check(full, ref, vq, tv, step + 1)
        assert torch.equal(out, full.to(TD[dtype]).reshape(1, 1, Hq * 128))  # the fp32 result rounded to the dtype
    assert cache.tails[2].capacity == 8
    # no per-token packed form and no file format for a gq layer
    for call in (lambda: cache.packed_nbytes(2), lambda: cache.dequantize(2), lambda: cache.save("unused.safetensors"),
                 lambda: cache.load("unused.safetensors")):
        with pytest.raises(ValueError, match="rtkv-gq/1"):
            call()
    with pytest.raises(ValueError):
        cache.attend(2, q[:, :, 0], H // 2)
    cache.store_group_quant(2, c)   # a new prefill drops the tail
    assert cache.tail_len(2) == 0
    tk, tv = make_tail(99, 0, F, dtype, spare=4)
    none = rtkv.DecodeTail.from_tensors(tk, tv, torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert torch.equal(cache.attend(2, q[:, :, 0], H), c.attend(q[:, :, 0]))   # no tail: today's path
    check(c.attend(q[:, :, 0], tail=none), reference(kq, vq, c.rows, tk, tv, 0, q[:, :, 0], H), vq, tv, 0)


def test_attend_chunk_is_causal_single_steps():
    """T = 3 new tokens over a gq layer with 5 older tail rows: query t sees the gq rows and tail rows
    u < 5 + t + 1."""
    import rtkv
    dtype, H, Hq, S, T, old = "bfloat16", 4, 8, 1300, 3, 5
    F = H * 128
    c, kq, vq, _, _ = layer(dtype, S, H, 4)
    cache = rtkv.CompressedKVCache(1, S, 128, tail_capacity=4)
    cache.store_group_quant(0, c)
    with pytest.raises(ValueError):
        cache.attend_chunk(0, rand(1, (1, Hq, T, 128), dtype), H)   # nothing appended yet
    tk, tv = rand(51, (1, old + T, F), dtype), rand(52, (1, old + T, F), dtype)
    cache.append(0, tk[:, :old], tv[:, :old])
    cache.append(0, tk[:, old:], tv[:, old:])
    q = rand(53, (1, Hq, T, 128), dtype)
    out = cache.attend_chunk(0, q, H)
    assert out.shape == (1, Hq, T, 128) and out.dtype == torch.float32
    for t in range(T):
        ref = reference(kq, vq, c.rows, tk, tv, old + t + 1, q[:, :, t].contiguous(), H)
        check(out[:, :, t], ref, vq, tv, old + t + 1)
    # the module form appends and attends
    cache.store_group_quant(0, c)
    cache.append(0, tk[:, :old], tv[:, :old])
    ext = rtkv.CompressedExtendAttention(cache, Hq, H, 128, 0)
    kn = tk[:, old:].view(1, T, H, 128).transpose(1, 2)
    vn = tv[:, old:].view(1, T, H, 128).transpose(1, 2)
    got = ext(q, kn, vn)
    assert torch.equal(got, out.to(TD[dtype]).transpose(1, 2).reshape(1, T, Hq * 128))


def test_cache_from_a_side_stream_needs_no_sync():
    """gq_compress(..., stream=) packs on a side stream; attend(tail=) waits for it on the device."""
    import rtkv
    dtype, H, Hq, S = "float16", 8, 8, 2000
    F = H * 128
    c, kq, vq, Kd, Vd = layer(dtype, S, H, 4)
    q = rand(61, (1, Hq, 128), dtype)
    T = 9
    tk, tv = make_tail(62, T, F, dtype)
    tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([T], device="cuda"))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    c2 = rtkv.gq_compress(Kd, Vd, c.kept_index, c.labels, c.row_offset, c.stats, c.rows, c.codes_k.numel(), c.bits,
                          c.cfg, stream=side)
    out = c2.attend(q, tail=tail)   # no explicit synchronisation in between
    check(out, reference(kq, vq, c.rows, tk, tv, T, q, H), vq, tv, T)
    assert torch.equal(out, c.attend(q, tail=tail))
