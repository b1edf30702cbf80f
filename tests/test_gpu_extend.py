"""GPU: attention of T new tokens over a packed layer followed by the dense tail
(rtkv_extend_attention_packed_tail, extend.hip) against plain PyTorch float64 attention per (b, t) over
cat(K'[:r_b], tail[:vis(b,t)]), vis(b,t) = max(0, n_b − (T−1−t)), K'/V' from compress_layer_kv_cache.
The ground truth never comes from the code under test.

Tolerance.  The error sources of tests/test_gpu_decode.py (fp32 summation order, hardware exp2) plus
one: the softmax weights pᵢ are rounded to the K/V dtype before the weights·V product on the matrix
core (their sum stays fp32).  That moves output element d of a query by at most u·Σᵢ pᵢ|vᵢd| = u·A_d,
u = 2⁻¹¹ (float16) or 2⁻⁸ (bfloat16), A = softmax(...)·|Y| the weighted mean of |V| in that channel under
the same visibility mask.  So, elementwise (tests/attn_checks.py has the derivation and the reference),

    |out − ref| ≤ 2e-4·|ref| + 2e-5·vmax + 2u·A,      vmax = max(max|V'|, max|tail V|, 1);

the factor 2 covers float16 underflow of very small weights and the lazily trailing maximum.  A ≤ vmax,
so this is nowhere looser than the (2e-5 + 2u)·vmax this file used before.  The float32 fallback (single
decode steps, no rounding of the weights, u = 0) keeps the decode tests' 2e-5·vmax.  check() prints the
worst |err| / bound of each comparison.  The largest seen on an MI355X: float16 0.30, bfloat16 0.35, both in
test_tail_only's 70-token chunk, whose first queries see two or three keys, so that the roundings of their
weights do not average out; the ground-truth cases stay at 0.06 (float16) and 0.07 (bfloat16), the CPU
emulation of tests/test_attn_bound_host.py at 0.09 and 0.10; float32 0.001.

Every unused tail row (capacity is always above the count) is NaN: a finite output within tolerance
shows that nothing at or past a count is read.

The queries of the ground-truth cases carry a multiple of the keys at the two ends of what each query sees
(attn_checks.plant_boundaries): without it a single row lost there is below the bfloat16 bound at about half of the steps."""
import ctypes

import pytest
import torch

from attn_checks import (QMUL, SHAPES, STEPS, Ref, check_bound, check_onehot, chunk_reference, onehot_tail,
                         plant_boundaries, visible)
from test_gpu_decode_tail import (SINGLE_ATOL, SINGLE_RTOL, TD, aimed_query, empty_packed, kept_classes, layer, lead,
                                  make_tail, rand, single_rows, swapped)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    import rtkv
    rtkv.build()


reference = chunk_reference   # Ref(out, A) in float64 per (b, t), the counts clamped as the kernel clamps them


def at(ref, *idx):
    return Ref(ref.out[idx], ref.A[idx])


def vmax_of(v2, tv, trows):
    cap = tv.shape[1]
    used = [min(max(int(t), 0), cap) for t in trows]
    tmax = max([tv[b, :t].float().abs().max().item() for b, t in enumerate(used) if t] + [0.0])
    return max(v2.float().abs().max().item() if v2.numel() else 0.0, tmax, 1.0)


def check(out, ref, v2, tv, trows, dtype, what=""):
    return check_bound(out, ref, vmax_of(v2, tv, trows), dtype, what)


# SHAPES and STEPS: attn_checks (tests/test_attn_bound_host.py runs the same ones on the CPU).  The 16-bit field
# width (by_width<16>) is that of a 15-bit class: with 16 bits a bfloat16 layer packs 17-bit fields, which the
# kernel refuses (test_gpu_decode_tail.test_17_bit_fields_are_refused), and a float16 layer is outside what the
# quantizer accepts (tests/test_gpu_parity.py).
CASES = [(s, dt, bits, STEPS[i]) for i, s in enumerate(SHAPES)
         for dt, bits in (("float16", (2, 4, 8)), ("bfloat16", (2, 4, 8)), ("bfloat16", (4, 8, 15)),
                          ("float16", (4, 8, 15)))]


def case_id(s, dt, bits):
    return f"{s[0]}-{s[1]}-{s[3]}-{dt}" + ("" if bits == (2, 4, 8) else "-" + "-".join(map(str, bits)))


@pytest.mark.parametrize("shape,dtype,bits,steps", CASES, ids=[case_id(s, dt, b) for s, dt, b, _ in CASES])
def test_ground_truth(shape, dtype, bits, steps):
    import rtkv
    S, Hkv, D, Hq = shape
    F = Hkv * D
    k2, v2, pk = layer(1, S, Hkv, D, dtype, bits)
    for T, older in steps:
        n = T + older
        q = rand(S + T, (1, Hq, T, D), dtype, QMUL)
        tk, tv = make_tail(S + 10 * n, 1, n, F, dtype)
        q[0] = plant_boundaries(q[0], k2[0], int(pk["rows"][0]), tk[0], n, Hkv, TD[dtype])
        tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([n]))
        out = rtkv.extend_attention(pk, q, Hkv, tail)
        assert out.shape == (1, Hq, T, D) and out.dtype == torch.float32
        ref = reference(k2, v2, pk["rows"], tk, tv, [n], q, Hkv, 1.0 / D ** 0.5)
        check(out, ref, v2, tv, [n], dtype, f"T {T} older {older}")
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
    A = reference(k2, v2, pk["rows"], tk, tv, [n], q, Hkv, 1.0 / D ** 0.5).A
    for t in range(T):
        one = rtkv.decode_attention(pk, q[:, :, t].contiguous(), Hkv,
                                    tail=rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([n - (T - 1 - t)])))
        check(out[:, :, t], Ref(one.double(), A[:, :, t]), v2, tv, [n], dtype, f"t {t}")


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
        check(out[:, :, t], at(ref, slice(None), slice(None), t), v2, tv, [n], dtype, f"t {t}")
    check(out, ref, v2, tv, [n], dtype)
    v3 = tv[0, older + 3, h * D:(h + 1) * D].float()
    assert (out[0, hq, 2] - v3).abs().max() > 0.5                          # query 2 is not on token 3's value
    # the other way: the key in query 2's own row
    tk, tv = make_tail(114, 1, n, F, dtype)
    tk[0, older + 2, h * D:(h + 1) * D] = q[0, hq, 2]
    tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([n]))
    out = rtkv.extend_attention(pk, q, Hkv, tail)
    check(out, reference(k2, v2, pk["rows"], tk, tv, [n], q, Hkv, 1.0 / D ** 0.5), v2, tv, [n], dtype)
    own = tv[0, older + 2, h * D:(h + 1) * D].double()                     # the whole weight: A = |V| of that row
    check(out[0, hq, 2], Ref(own, own.abs()), v2, tv, [n], dtype, "own row")


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_batch_of_two_with_strided_tail(dtype):
    """Different kept counts per row, tail counts [T, T + 7], a batch stride larger than capacity · F."""
    import rtkv
    B, S, Hkv, D, Hq, T = 2, 800, 8, 128, 32, 6
    F = Hkv * D
    k2, v2, pk0 = layer(B, S, Hkv, D, dtype)
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
            first = tv[0, 0].double().view(Hkv, 1, D).expand(Hkv, G, D).reshape(Hq, D)
            check(out[0, :, 0], Ref(first, first.abs()), v2[:, :0], tv, [1], dtype, "query 0")


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


@pytest.mark.parametrize("dtype,bits", [("float16", (2, 4, 8)), ("bfloat16", (2, 4, 8)), ("bfloat16", (4, 8, 15)),
                                        ("float16", (4, 8, 15))],
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_one_packed_row_takes_the_whole_weight(dtype, bits):
    """q of one (query head, t) a multiple of K'[r] of its kv head: that query's output is V'[r], for one row
    of each class (each field width: by_width<2 / 4 / 8 / 16>), the last kept row (its width comes from its
    label) and the first row of a later split — and the same with K and V exchanged, where the output is
    K'[r].  The in-kernel decode (for float16 (h − zp)·sc in half arithmetic) is thereby compared element for
    element with the K'/V' that compress_layer_kv_cache wrote.  Tolerance: test_gpu_decode_tail.SINGLE_RTOL."""
    import rtkv
    S, Hkv, D, Hq = 620, 4, 128, 8
    F, G, T, older, hq, t = Hkv * D, Hq // Hkv, 5, 3, 5, 3
    h, nt = hq // G, T + older
    k2, v2, pk = layer(1, S, Hkv, D, dtype, bits)
    n = int(pk["rows"][0])
    tk, tv = make_tail(302, 1, nt, F, dtype)
    tail = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([nt]))
    seen = int(visible(T, nt)[t])
    for p, X, Y in ((pk, k2, v2), (swapped(pk), v2, k2)):
        Xh = X[0, :n, h * D:(h + 1) * D]
        vmax = max(Y[0, :n].float().abs().max().item(), tv[:, :nt].float().abs().max().item(), 1.0)
        for name, r in single_rows(pk).items():
            q = rand(303, (1, Hq, T, D), dtype)
            q[0, hq, t] = aimed_query(Xh, r, D, dtype)
            top, by = lead(torch.cat([Xh, tk[0, :seen, h * D:(h + 1) * D]]), q[0, hq, t], D)
            assert top == r and by > 30, (name, r, top, by)
            out = rtkv.extend_attention(p, q, Hkv, tail)
            row = Y[0, r, h * D:(h + 1) * D].float()
            err = (out[0, hq, t] - row).abs().max().item()
            print(f"{name} (row {r} of {n}, class {int(kept_classes(pk)[r])}): lead {by:.1f} nats, "
                  f"max |out - row| {err:.2e}")
            torch.testing.assert_close(out[0, hq, t], row, rtol=SINGLE_RTOL, atol=SINGLE_ATOL * vmax,
                                       msg=lambda m: f"{name}: {m}")


# (dtype, T, G, tail counts per batch row, spare NaN rows, counts on the device as given).  Hkv = 4 (B = 1) or 8
# (B = 2), D = 128.  Counts around the 32-key image (31, 32, 33), around four waves' images and the rows of a
# split (127, 128, 129), around a second split (255, 257), several tail splits (1570); G·T below, at and above
# 16 (one or two query tiles per pass) and above 32 (several passes): passes inside one GQA head (G = 4, T = 70)
# and passes that span two (G = 2, T = 17); B = 2 with different counts and a strided tail; device-side
# counts below T, zero, above the capacity and negative (the expectation clamps as the kernel must).
MAPS = [
    ("float16", 1, 1, [31], 3, None),
    ("bfloat16", 5, 2, [32], 3, None),
    ("float16", 16, 1, [33], 3, None),
    ("bfloat16", 17, 2, [127], 1, None),
    ("float16", 33, 1, [128], 1, None),
    ("bfloat16", 70, 4, [129], 3, None),
    ("float16", 5, 4, [255], 1, None),
    ("bfloat16", 17, 1, [257], 3, None),
    ("float16", 70, 2, [1570], 3, None),
    ("bfloat16", 16, 4, [1570], 2, None),
    ("float16", 33, 2, [129, 40], 5, None),
    ("bfloat16", 70, 1, [64, 257], 3, None),
    ("float16", 17, 2, [5, 0], 130, [5, 0]),
    ("bfloat16", 33, 4, [130, 0], 0, [1130, -4]),
]


@pytest.mark.parametrize("dtype,T,G,counts,spare,device_counts", MAPS,
                         ids=[f"{dt}-T{T}-G{G}-" + "-".join(map(str, dc or c)) for dt, T, G, c, _, dc in MAPS])
def test_onehot_tail_map(dtype, T, G, counts, spare, device_counts):
    """Zero keys and one-hot values (attn_checks.onehot_tail) and no packed row: every logit is 0, every
    weight exactly 1 in fp32 and in the dtype, every sum a small integer, so
    out[b, hq, t, c] = #{u < vis(b, t) : u mod 128 = c} / vis(b, t) with no tolerance: zeros exactly zero, the
    rest within one float32 ulp (check_onehot).  A tail row skipped, read twice or shown to a query one step
    early or late shows in its channel, at every position.  Unused rows are NaN."""
    import rtkv
    B, D = len(counts), 128
    Hkv = 4 if B == 1 else 8
    Hq, cap = Hkv * G, max(counts) + spare
    k2, v2, pk0 = layer(B, 620 if B == 1 else 800, Hkv, D, dtype)
    none = {k: v for k, v in pk0.items() if k != "_rows_dev"}
    none["rows"] = [0] * B
    tk, tv = onehot_tail(B, cap, Hkv, D, TD[dtype], counts, "cuda", spare=4 if B > 1 else 0)
    assert B == 1 or tk.stride(0) > cap * Hkv * D
    rows = torch.tensor(counts) if device_counts is None else torch.tensor(device_counts, device="cuda")
    tail = rtkv.DecodeTail.from_tensors(tk, tv, rows)
    vis = torch.stack([visible(T, n) for n in counts])[:, None, :]          # [B, 1, T]
    q = rand(311 + T, (B, Hq, T, D), dtype)
    for name, p in (("rows = [0]", none), ("no packed capacity", empty_packed(B, Hkv * D, dtype))):
        out = rtkv.extend_attention(p, q, Hkv, tail)
        assert out.shape == (B, Hq, T, D)
        check_onehot(out, vis, name)
