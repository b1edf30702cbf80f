"""GPU: attention of T new tokens over a packed layer followed by the dense tail
(rtkv_extend_attention_packed_tail, extend.hip) against plain PyTorch fp32 attention per (b, t) over
cat(K'[:r_b], tail[:vis(b,t)]), vis(b,t) = max(0, n_b − (T−1−t)), K'/V' from compress_layer_kv_cache.
The ground truth never comes from the code under test.

Tolerance.  The error sources of tests/test_gpu_decode.py (fp32 summation order, hardware exp2) plus
one: the softmax weights are rounded to the K/V dtype before the weights·V product on the matrix
core (their sum stays fp32), which perturbs the output by at most u·max|V|, u = 2⁻¹¹ (float16) or
2⁻⁸ (bfloat16).  So rtol = 2e-4, atol = (2e-5 + 2u)·vmax with vmax = max(max|V'|, max|tail V|, 1);
the factor 2 covers float16 underflow of very small weights and the lazily trailing maximum.  The
float32 fallback (single decode steps, no rounding of the weights) keeps the decode tests' 2e-5·vmax.

Every unused tail row (capacity is always above the count) is NaN: a finite output within tolerance
shows that nothing at or past a count is read."""
import ctypes

import pytest
import torch

from test_gpu_decode_tail import TD, empty_packed, layer, make_tail, rand

pytestmark = pytest.mark.gpu

U = {"float16": 2.0 ** -11, "bfloat16": 2.0 ** -8, "float32": 0.0}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    import rtkv
    rtkv.build()


def reference(k2, v2, rows, tk, tv, trows, q, Hkv, scale):
    """fp32 softmax(q_t·Xᵀ·scale)·Y per (b, t): X/Y = cat(K'/V'[:rows[b]], tail[:vis(b, t)])."""
    B, Hq, T, D = q.shape
    G = Hq // Hkv
    cap = tk.shape[1]
    out = torch.zeros(B, Hq, T, D, dtype=torch.float32, device=q.device)
    for b in range(B):
        n, nb = int(rows[b]), min(max(int(trows[b]), 0), cap)
        if n + nb == 0:
            continue
        Kf = torch.cat([k2[b, :n].float(), tk[b, :nb].float()]).view(n + nb, Hkv, D)
        Vf = torch.cat([v2[b, :n].float(), tv[b, :nb].float()]).view(n + nb, Hkv, D)
        s = torch.einsum("hgtd,nhd->hgtn", q[b].float().view(Hkv, G, T, D), Kf) * scale
        vis = (nb - (T - 1 - torch.arange(T, device=q.device))).clamp(min=0)
        seen = torch.arange(n + nb, device=q.device)[None, :] < (n + vis)[:, None]        # [T, n + nb]
        p = torch.softmax(s.masked_fill(~seen, float("-inf")), dim=-1)
        p = torch.where(seen.any(1)[:, None], p, torch.zeros_like(p))                     # no visible key: zeros
        out[b] = torch.einsum("hgtn,nhd->hgtd", p, Vf).reshape(Hq, T, D)
    return out


def check(out, ref, v2, tv, trows, dtype):
    assert torch.isfinite(out).all()
    cap = tv.shape[1]
    used = [min(max(int(t), 0), cap) for t in trows]
    tmax = max([tv[b, :t].float().abs().max().item() for b, t in enumerate(used) if t] + [0.0])
    vmax = max(v2.float().abs().max().item() if v2.numel() else 0.0, tmax, 1.0)
    atol = (2e-5 + 2 * U[dtype]) * vmax
    err = (out - ref).abs().max().item()
    print(f"max |err| {err:.3e}  atol {atol:.3e}  vmax {vmax:.3f}")
    torch.testing.assert_close(out, ref, rtol=2e-4, atol=atol)


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
CASES = [(s, dt, STEPS[i]) for i, s in enumerate(SHAPES) for dt in ("float16", "bfloat16")]


@pytest.mark.parametrize("shape,dtype,steps", CASES, ids=[f"{s[0]}-{s[1]}-{s[3]}-{dt}" for s, dt, _ in CASES])
def test_ground_truth(shape, dtype, steps):
    import rtkv
    S, Hkv, D, Hq = shape
    F = Hkv * D
    k2, v2, pk = layer(1, S, Hkv, D, dtype, (2, 4, 8))
    for T, older in steps:
        n = T + older
        q = rand(S + T, (1, Hq, T, D), dtype)
        tk, tv = make_tail(S + 10 * n, 1, n, F, dtype)
        tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([n]))
        out = rtkv.extend_attention(pk, q, Hkv, tail)
        assert out.shape == (1, Hq, T, D) and out.dtype == torch.float32
        ref = reference(k2, v2, pk["rows"], tk, tv, [n], q, Hkv, 1.0 / D ** 0.5)
        check(out, ref, v2, tv, [n], dtype)
        assert torch.equal(rtkv.extend_attention(pk, q, Hkv, tail), out)   # deterministic


@pytest.mark.parametrize("shape,dtype", [(SHAPES[2], "float16"), (SHAPES[3], "bfloat16")])
def test_agrees_with_single_steps(shape, dtype):
    """Query t of a 5-token chunk against the existing single-token step over the tail up to token t."""
    import rtkv
    S, Hkv, D, Hq = shape
    T, n = 5, 5 + 9
    k2, v2, pk = layer(1, S, Hkv, D, dtype)
    q = rand(101, (1, Hq, T, D), dtype)
    tk, tv = make_tail(102, 1, n, Hkv * D, dtype)
    out = rtkv.extend_attention(pk, q, Hkv, rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([n])))
    for t in range(T):
        one = rtkv.decode_attention(pk, q[:, :, t].contiguous(), Hkv,
                                    tail=rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([n - (T - 1 - t)])))
        check(out[:, :, t], one, v2, tv, [n], dtype)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_no_causal_leak(dtype):
    """A tail key equal to query 2 of one head (|q|²/√D ≈ 16·√D, far above q·k of any other row) in the
    row of new token 3: query 2 must not see it, queries 3 and 4 see it as the ground truth says (it
    carries query 2, not their own).  The same key in query 2's own row takes that head's whole weight."""
    import rtkv
    S, Hkv, D, Hq = 620, 4, 128, 8
    F, G = Hkv * D, Hq // Hkv
    k2, v2, pk = layer(1, S, Hkv, D, dtype)
    T, older, hq = 5, 3, 5
    n, h = T + older, hq // G
    q = rand(111, (1, Hq, T, D), dtype, mul=4.0)
    tk, tv = make_tail(112, 1, n, F, dtype)
    tk[0, older + 3, h * D:(h + 1) * D] = q[0, hq, 2]
    tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([n]))
    out = rtkv.extend_attention(pk, q, Hkv, tail)
    ref = reference(k2, v2, pk["rows"], tk, tv, [n], q, Hkv, 1.0 / D ** 0.5)
    for t in (2, 3, 4):
        check(out[:, :, t], ref[:, :, t], v2, tv, [n], dtype)
    check(out, ref, v2, tv, [n], dtype)
    vmax = max(v2.float().abs().max().item(), tv[:, :n].float().abs().max().item(), 1.0)
    atol = (2e-5 + 2 * U[dtype]) * vmax
    v3 = tv[0, older + 3, h * D:(h + 1) * D].float()
    assert not torch.allclose(out[0, hq, 2], v3, rtol=2e-4, atol=atol)     # query 2 is not on token 3's value
    # the other way: the key in query 2's own row
    tk, tv = make_tail(114, 1, n, F, dtype)
    tk[0, older + 2, h * D:(h + 1) * D] = q[0, hq, 2]
    tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([n]))
    out = rtkv.extend_attention(pk, q, Hkv, tail)
    check(out, reference(k2, v2, pk["rows"], tk, tv, [n], q, Hkv, 1.0 / D ** 0.5), v2, tv, [n], dtype)
    torch.testing.assert_close(out[0, hq, 2], tv[0, older + 2, h * D:(h + 1) * D].float(), rtol=2e-4, atol=atol)


def test_batch_of_two_with_strided_tail():
    """Different kept counts per row, tail counts [T, T + 7], a batch stride larger than capacity · F."""
    import rtkv
    B, S, Hkv, D, Hq, dtype, T = 2, 800, 8, 128, 32, "float16", 6
    F = Hkv * D
    k2, v2, pk0 = layer(B, S, Hkv, D, dtype, ratio=0.5)
    pk = {k: v for k, v in pk0.items() if k != "_rows_dev"}
    pk["rows"] = [int(pk0["rows"][0]), int(pk0["rows"][1]) - 17]
    cap = T + 9
    big_k, big_v = make_tail(121, B, 0, F, dtype, spare=cap + 4)    # NaN everywhere
    tk, tv = big_k[:, :cap], big_v[:, :cap]
    for b, nb in enumerate((T, T + 7)):
        tk[b, :nb] = rand(122 + b, (nb, F), dtype)
        tv[b, :nb] = rand(124 + b, (nb, F), dtype)
    assert tk.stride(0) > cap * F
    tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([T, T + 7]))
    q = rand(126, (B, Hq, T, D), dtype)
    out = rtkv.extend_attention(pk, q, Hkv, tail)
    check(out, reference(k2, v2, pk["rows"], tk, tv, [T, T + 7], q, Hkv, 1.0 / D ** 0.5), v2, tv, [T, T + 7], dtype)
    # a strided q (the model's [B, T, Hq, D] projection output seen as [B, Hq, T, D]) gives the same bits
    qs = q.transpose(1, 2).contiguous().transpose(1, 2)
    assert not qs.is_contiguous() and torch.equal(rtkv.extend_attention(pk, qs, Hkv, tail), out)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_tail_only(dtype):
    """No packed row (rows = [0]) and no packed capacity at all: attention over the chunk alone.
    Query 0 sees one key, so its output is that row's V."""
    import rtkv
    S, Hkv, D, Hq = 620, 4, 128, 8
    F, G = Hkv * D, Hq // Hkv
    k2, v2, pk0 = layer(1, S, Hkv, D, dtype)
    none = {k: v for k, v in pk0.items() if k != "_rows_dev"}
    none["rows"] = [0]
    for T in (1, 70):
        q = rand(131 + T, (1, Hq, T, D), dtype)
        tk, tv = make_tail(132 + T, 1, T, F, dtype)
        tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([T]))
        ref = reference(k2[:, :0], v2[:, :0], [0], tk, tv, [T], q, Hkv, 1.0 / D ** 0.5)
        for p in (none, empty_packed(1, F, dtype)):
            out = rtkv.extend_attention(p, q, Hkv, tail)
            check(out, ref, v2[:, :0], tv, [T], dtype)
            first = tv[0, 0].float().view(Hkv, 1, D).expand(Hkv, G, D).reshape(Hq, D)
            torch.testing.assert_close(out[0, :, 0], first, rtol=2e-4, atol=(2e-5 + 2 * U[dtype]) * max(first.abs().max().item(), 1.0))


def test_short_tail():
    """A device-side tail count below T: vis = max(0, 3 − (4 − t)); with no packed row the queries
    that see nothing give zeros."""
    import rtkv
    S, Hkv, D, Hq, dtype, T = 700, 4, 128, 4, "float16", 5
    F = Hkv * D
    k2, v2, pk0 = layer(1, S, Hkv, D, dtype)
    q = rand(141, (1, Hq, T, D), dtype)
    tk, tv = make_tail(142, 1, 3, F, dtype, spare=4)
    tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([3], device="cuda"))
    out = rtkv.extend_attention(pk0, q, Hkv, tail)
    check(out, reference(k2, v2, pk0["rows"], tk, tv, [3], q, Hkv, 1.0 / D ** 0.5), v2, tv, [3], dtype)
    none = {k: v for k, v in pk0.items() if k != "_rows_dev"}
    none["rows"] = [0]
    out = rtkv.extend_attention(none, q, Hkv, tail)
    check(out, reference(k2[:, :0], v2[:, :0], [0], tk, tv, [3], q, Hkv, 1.0 / D ** 0.5), v2[:, :0], tv, [3], dtype)
    assert torch.count_nonzero(out[:, :, :2]) == 0 and torch.count_nonzero(out[:, :, 2]) > 0
    # a count above the capacity is clamped to it, a negative one to 0
    over = rtkv.DecodeTail.from_tensors(tk[:, :3], tv[:, :3], torch.tensor([1000], device="cuda"))
    assert torch.equal(rtkv.extend_attention(none, q, Hkv, over), out)
    neg = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([-4], device="cuda"))
    assert torch.count_nonzero(rtkv.extend_attention(none, q, Hkv, neg)) == 0


def test_rejected_input_and_fallback():
    """float32 and head_dim 64 are outside the kernel's envelope (RTKV_ERR_UNSUPPORTED through the C
    entry point); the Python call still answers, through single decode steps."""
    import rtkv
    import rtkv._lib as L
    T = 3
    rows_dev = torch.tensor([T], device="cuda")
    for dt, tdt, Hkv, D in ((L.F32, torch.float32, 4, 128), (L.F16, torch.float16, 8, 64)):
        Hq, F = Hkv, Hkv * D
        q = torch.zeros(1, Hq, T, D, dtype=tdt, device="cuda")
        tk = torch.zeros(1, 8, F, dtype=tdt, device="cuda")
        out = torch.zeros(1, Hq, T, D, device="cuda")
        n = L.lib().rtkv_extend_workspace_size(1, Hq, Hkv, D, T, 0, 8)
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        tail = L.DenseTail(tk.data_ptr(), tk.data_ptr(), rows_dev.data_ptr(), 8, tk.stride(0), tk.stride(1))
        rc = L.lib().rtkv_extend_attention_packed_tail(0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, Hkv, D, dt, None, q.data_ptr(),
                                                       q.stride(0), q.stride(1), q.stride(2), Hq, T, 0.1,
                                                       ctypes.byref(tail), out.data_ptr(), ws.data_ptr(), n,
                                                       L.stream_ptr(q.device))
        assert rc == -2 and "extend: " in L.lib().rtkv_last_error().decode()     # RTKV_ERR_UNSUPPORTED
    S, Hkv, D, Hq, dtype = 700, 4, 128, 4, "float32"
    k2, v2, pk = layer(1, S, Hkv, D, dtype)
    n = T + 4
    q = rand(151, (1, Hq, T, D), dtype)
    tk, tv = make_tail(152, 1, n, Hkv * D, dtype)
    out = rtkv.extend_attention(pk, q, Hkv, rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([n])))
    check(out, reference(k2, v2, pk["rows"], tk, tv, [n], q, Hkv, 1.0 / D ** 0.5), v2, tv, [n], dtype)
    with pytest.raises(ValueError):
        rtkv.extend_attention(pk, q.half(), Hkv, rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([n])))
    torch.cuda.synchronize()


def test_module_loop():
    """store_packed, a 6-token chunk, three single decode steps, a 4-token chunk on one cache: every
    output against torch over the growing cache."""
    import rtkv
    B, S, Hkv, D, Hq, dtype = 1, 512, 8, 128, 32, "float16"
    F = Hkv * D
    k2, v2, pk = layer(B, S, Hkv, D, dtype)
    cache = rtkv.CompressedKVCache(B, S, D, tail_capacity=4)
    cache.store_packed(2, pk)
    chunk = rtkv.CompressedExtendAttention(cache, Hq, Hkv, D, 2)
    one = rtkv.CompressedDecodeAttention(cache, Hq, Hkv, D, 2)
    ks, vs = [], []
    for step, T in enumerate((6, 1, 1, 1, 4)):
        q = rand(160 + step, (B, Hq, T, D), dtype)
        k = rand(170 + step, (B, Hkv, T, D), dtype)
        v = rand(180 + step, (B, Hkv, T, D), dtype)
        out = (one if T == 1 and step else chunk)(q, k, v)
        assert out.shape == (B, T, Hq * D) and out.dtype == TD[dtype]
        ks.append(k.transpose(1, 2).reshape(B, T, F))
        vs.append(v.transpose(1, 2).reshape(B, T, F))
        tk, tv = torch.cat(ks, 1), torch.cat(vs, 1)
        n = tk.shape[1]
        assert cache.tail_len(2) == n
        ref = reference(k2, v2, pk["rows"], tk, tv, [n], q, Hkv, 1.0 / D ** 0.5)
        full = cache.attend_chunk(2, q, Hkv)
        check(full, ref, v2, tv, [n], dtype)
        if T > 1:
            assert torch.equal(out, full.to(TD[dtype]).transpose(1, 2).reshape(B, T, Hq * D))
        else:
            check(out.float().view(B, Hq, 1, D), ref, v2, tv, [n], dtype)   # the result rounded to the query dtype
    assert cache.tail_len(2) == 13
    with pytest.raises(ValueError):
        chunk(q, k, v, attention_mask=torch.zeros(B, 1, 4, 4, device="cuda"))
    assert cache.tail_len(2) == 13
