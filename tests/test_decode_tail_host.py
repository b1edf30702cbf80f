"""CPU: the host side of the decode tail (rtkv.DecodeTail) — the dense K/V rows of the tokens
generated after a compressed prefill (the reference concatenates them onto the cache,
modified_llama.py:83-94).  Appending, growth and the validation of caller-owned buffers are plain
torch and run on CPU tensors; attention itself has no CPU path and must say so."""
import pytest
import torch


def rows(B, T, F, seed, dtype=torch.float16):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, T, F, generator=g).to(dtype)


def test_append_single_rows_and_blocks():
    import rtkv
    B, F = 2, 512
    t = rtkv.DecodeTail(B, F, torch.float16, "cpu", capacity=8)
    assert t.capacity == 8 and len(t) == 0 and t.rows_dev.dtype == torch.int64 and t.rows_dev.tolist() == [0, 0]
    k1, v1 = rows(B, 1, F, 1), rows(B, 1, F, 2)
    t.append(k1[:, 0], v1[:, 0])                       # [B, F]
    k3, v3 = rows(B, 3, F, 3), rows(B, 3, F, 4)
    t.append(k3, v3)                                   # [B, 3, F]
    assert len(t) == 4 and t.rows_dev.tolist() == [4, 4] and t.capacity == 8
    assert torch.equal(t.k[:, :4], torch.cat([k1, k3], 1)) and torch.equal(t.v[:, :4], torch.cat([v1, v3], 1))
    assert t.k.shape == (B, 8, F) and t.k.dtype == torch.float16


def test_growth_keeps_contents_and_counts():
    import rtkv
    B, F = 2, 512
    t = rtkv.DecodeTail(B, F, torch.bfloat16, "cpu", capacity=4)
    K, V = rows(B, 9, F, 5, torch.bfloat16), rows(B, 9, F, 6, torch.bfloat16)
    caps = []
    for i in range(9):
        t.append(K[:, i], V[:, i])
        caps.append(t.capacity)
        assert len(t) == i + 1 and t.rows_dev.tolist() == [i + 1] * B
        assert torch.equal(t.k[:, :i + 1], K[:, :i + 1]) and torch.equal(t.v[:, :i + 1], V[:, :i + 1])
    assert caps == [4, 4, 4, 4, 8, 8, 8, 8, 16]       # doubled when full
    # a block that needs more than one doubling
    t2 = rtkv.DecodeTail(1, F, torch.float32, "cpu", capacity=4)
    blk = rows(1, 19, F, 7, torch.float32)
    t2.append(blk, blk)
    assert t2.capacity == 32 and len(t2) == 19 and torch.equal(t2.k[:, :19], blk)


def test_append_rejects_mismatched_input():
    import rtkv
    t = rtkv.DecodeTail(2, 512, torch.float16, "cpu", capacity=4)
    ok = rows(2, 1, 512, 1)
    with pytest.raises(ValueError):
        t.append(ok.float(), ok.float())               # dtype
    with pytest.raises(ValueError):
        t.append(rows(3, 1, 512, 1), rows(3, 1, 512, 1))   # B
    with pytest.raises(ValueError):
        t.append(rows(2, 1, 256, 1), rows(2, 1, 256, 1))   # F
    with pytest.raises(ValueError):
        t.append(ok, rows(2, 2, 512, 1))               # K and V disagree
    with pytest.raises(ValueError):
        t.append(ok.to("meta"), ok.to("meta"))         # device
    assert len(t) == 0 and t.rows_dev.tolist() == [0, 0]
    with pytest.raises(ValueError):
        rtkv.DecodeTail(2, 512, torch.int8, "cpu")


def test_from_tensors_wraps_and_validates():
    import rtkv
    B, cap, F = 2, 6, 512
    k, v = rows(B, cap, F, 8), rows(B, cap, F, 9)
    t = rtkv.DecodeTail.from_tensors(k, v, torch.tensor([0, 5]))
    assert t.k is k and t.v is v and t.capacity == cap and t.rows_dev.tolist() == [0, 5]
    with pytest.raises(ValueError):
        t.append(k[:, :1], v[:, :1])                   # caller-owned: not appendable
    # a batch stride larger than capacity·F
    big_k, big_v = rows(B, cap + 2, F, 10), rows(B, cap + 2, F, 11)
    t = rtkv.DecodeTail.from_tensors(big_k[:, :cap], big_v[:, :cap], torch.tensor([6, 1]))
    assert t.k.stride(0) == (cap + 2) * F
    with pytest.raises(ValueError, match="outside"):
        rtkv.DecodeTail.from_tensors(k, v, torch.tensor([0, cap + 1]))      # a count above capacity
    with pytest.raises(ValueError, match="outside"):
        rtkv.DecodeTail.from_tensors(k, v, torch.tensor([-1, 0]))
    with pytest.raises(ValueError):
        rtkv.DecodeTail.from_tensors(k, v, torch.tensor([0, 1], dtype=torch.int32))   # rows dtype
    with pytest.raises(ValueError):
        rtkv.DecodeTail.from_tensors(k, v.float(), torch.tensor([0, 1]))    # K and V dtypes differ
    with pytest.raises(ValueError):
        rtkv.DecodeTail.from_tensors(k.to(torch.int16), v.to(torch.int16), torch.tensor([0, 1]))
    with pytest.raises(ValueError):
        rtkv.DecodeTail.from_tensors(k, v, torch.tensor([0, 1, 2]))         # B
    with pytest.raises(ValueError):
        rtkv.DecodeTail.from_tensors(k, v[:, :, :256], torch.tensor([0, 1]))  # F
    # rows of 516 halves = 1032 bytes: every second row is only 8-byte aligned
    wide_k, wide_v = rows(B, cap, 516, 12), rows(B, cap, 516, 13)
    with pytest.raises(ValueError, match="aligned"):
        rtkv.DecodeTail.from_tensors(wide_k[:, :, :512], wide_v[:, :, :512], torch.tensor([1, 1]))
    # a base pointer 8 bytes into a row
    with pytest.raises(ValueError, match="aligned"):
        rtkv.DecodeTail.from_tensors(rows(B, cap, 520, 14)[:, :, 4:516], rows(B, cap, 520, 15)[:, :, 4:516],
                                     torch.tensor([1, 1]))
    # transposed storage: no unit stride along F
    with pytest.raises(ValueError):
        rtkv.DecodeTail.from_tensors(rows(B, F, cap, 16).transpose(1, 2), rows(B, F, cap, 17).transpose(1, 2),
                                     torch.tensor([1, 1]))


def packed_stub(B, F, dtype):
    """A packed layer dict with no kept row (the shapes decode_attention checks)."""
    return {"codes_k": torch.zeros(0, dtype=torch.uint8), "codes_v": torch.zeros(0, dtype=torch.uint8),
            "row_offset": torch.zeros(B, 0, dtype=torch.int64), "scale_zp": torch.zeros(B, 0, 4),
            "kept_index": torch.zeros(B, 0, dtype=torch.int32), "labels": torch.zeros(B, 8, dtype=torch.uint8),
            "rows": [0] * B, "bits": (2, 4, 8), "dtype": dtype, "feature_dim": F}


def test_attention_has_no_cpu_path():
    import rtkv
    B, F, Hkv, D = 1, 512, 4, 128
    t = rtkv.DecodeTail(B, F, torch.float16, "cpu", capacity=4)
    t.append(rows(B, 1, F, 1), rows(B, 1, F, 2))
    q = torch.zeros(B, Hkv, D, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="ROCm"):
        rtkv.decode_attention(packed_stub(B, F, torch.float16), q, Hkv, tail=t)


def test_cache_tail_bookkeeping():
    """CompressedKVCache.append creates the layer's tail from the packed layer's dtype, F and B;
    tail_len counts the appended tokens; store_packed and clear_cache drop the tail."""
    import rtkv
    B, F = 2, 512
    cache = rtkv.CompressedKVCache(B, 64, 128, tail_capacity=4)
    cache.store_packed(3, packed_stub(B, F, torch.bfloat16))
    assert cache.tail_len(3) == 0
    for i in range(6):
        cache.append(3, rows(B, 1, F, i, torch.bfloat16), rows(B, 1, F, 50 + i, torch.bfloat16))
        assert cache.tail_len(3) == i + 1
    t = cache.tails[3]
    assert t.k.dtype == torch.bfloat16 and t.k.shape == (B, 8, F) and t.rows_dev.tolist() == [6, 6]
    with pytest.raises(ValueError):
        cache.append(3, rows(B, 1, F, 0), rows(B, 1, F, 0))     # fp16 rows into a bf16 layer
    cache.store_packed(3, packed_stub(B, F, torch.bfloat16))
    assert cache.tail_len(3) == 0 and 3 not in cache.tails
    cache.append(3, rows(B, 2, F, 1, torch.bfloat16), rows(B, 2, F, 2, torch.bfloat16))
    assert cache.tail_len(3) == 2
    cache.clear_cache()
    assert not cache.tails and not cache.compression_info


def test_decode_module_rejects_masks_and_shapes():
    import rtkv
    B, Hq, Hkv, D = 1, 8, 4, 128
    cache = rtkv.CompressedKVCache(B, 64, D)
    cache.store_packed(0, packed_stub(B, Hkv * D, torch.float16))
    att = rtkv.CompressedDecodeAttention(cache, Hq, Hkv, D, 0)
    q = torch.zeros(B, Hq, 1, D, dtype=torch.float16)
    kv = torch.zeros(B, Hkv, 1, D, dtype=torch.float16)
    with pytest.raises(ValueError, match="mask"):
        att(q, kv, kv, attention_mask=torch.zeros(B, 1, 1, 1))
    with pytest.raises(ValueError):
        att(torch.zeros(B, Hq, 2, D, dtype=torch.float16), kv, kv)
    assert cache.tail_len(0) == 0                       # nothing was appended by the rejected calls
    with pytest.raises(RuntimeError, match="ROCm"):     # appends, then attention has no CPU path
        att(q, kv, kv)
    assert cache.tail_len(0) == 1
