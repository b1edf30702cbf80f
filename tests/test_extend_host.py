"""CPU: the host side of the multi-token step over the packed cache
(rtkv_extend_attention_packed_tail, rtkv.CompressedExtendAttention): the workspace size, the argument
checks the library makes before any launch, and the module's validation and tail bookkeeping.
Attention itself has no CPU path and must say so."""
import ctypes

import pytest
import torch


def packed_stub(B, F, dtype):
    """A packed layer dict with no kept row (the shapes extend_attention checks)."""
    return {"codes_k": torch.zeros(0, dtype=torch.uint8), "codes_v": torch.zeros(0, dtype=torch.uint8),
            "row_offset": torch.zeros(B, 0, dtype=torch.int64), "scale_zp": torch.zeros(B, 0, 4),
            "kept_index": torch.zeros(B, 0, dtype=torch.int32), "labels": torch.zeros(B, 8, dtype=torch.uint8),
            "rows": [0] * B, "bits": (2, 4, 8), "dtype": dtype, "feature_dim": F}


def test_workspace_size_is_positive_and_monotone():
    import rtkv._lib as L
    size = L.lib().rtkv_extend_workspace_size
    for B, Hq, Hkv in ((1, 4, 4), (1, 32, 8), (2, 32, 32), (3, 8, 4)):
        for cap, tcap in ((0, 0), (0, 5), (700, 0), (700, 64), (16384, 1024), (16384, 4096)):
            prev = 0
            for T in (1, 2, 5, 16, 17, 31, 32, 33, 64, 65, 70, 128, 129, 256, 1000):
                n = size(B, Hq, Hkv, 128, T, cap, tcap)
                assert n > 0 and n >= prev, (B, Hq, Hkv, cap, tcap, T, n, prev)
                prev = n
        for T in (1, 16, 70, 256):
            prev = 0
            for cap in (0, 1, 127, 128, 129, 1000, 5000, 16384, 65536, 200000):
                n = size(B, Hq, Hkv, 128, T, cap, 256)
                assert n > 0 and n >= prev
                prev = n
            prev = 0
            for tcap in (0, 1, 4, 127, 128, 129, 256, 1024, 4096, 100000):
                n = size(B, Hq, Hkv, 128, T, 16384, tcap)
                assert n > 0 and n >= prev
                prev = n


def test_entry_point_checks_arguments_on_the_host():
    """Every one of these is refused before anything touches a device: the pointers are made up."""
    import rtkv._lib as L
    lib = L.lib()
    Hq, Hkv, D, T, tcap = 8, 4, 128, 4, 16
    F = Hkv * D
    fake = 1 << 20                                       # 16-byte aligned, never dereferenced
    ws_bytes = lib.rtkv_extend_workspace_size(1, Hq, Hkv, D, T, 0, tcap)
    good = L.DenseTail(fake, fake, fake, tcap, tcap * F, F)

    def call(tail=good, T=T, qst=D, q=fake, nbytes=ws_bytes, dtype=L.F16):
        return lib.rtkv_extend_attention_packed_tail(0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, Hkv, D, dtype, None, q, Hq * T * D,
                                                     T * D, qst, Hq, T, 0.1, ctypes.byref(tail), fake, fake, nbytes,
                                                     None)
    for rc in (call(T=0),
               call(T=-3),
               call(tail=L.DenseTail(fake, fake, 0, tcap, tcap * F, F)),          # null rows_dev
               call(tail=L.DenseTail(fake, fake, fake, -1, tcap * F, F)),         # negative capacity
               call(tail=L.DenseTail(fake + 8, fake, fake, tcap, tcap * F, F)),   # misaligned tail base
               call(tail=L.DenseTail(fake, fake, fake, tcap, tcap * F, F + 4)),   # misaligned tail stride
               call(qst=D + 4),                                                   # misaligned q stride
               call(q=fake + 8),                                                  # misaligned q
               call(nbytes=ws_bytes - 1024),
               call(nbytes=0)):
        assert rc == -1                                                           # RTKV_ERR_INVALID
        assert "extend: " in lib.rtkv_last_error().decode()


def test_extend_attention_has_no_cpu_path():
    import rtkv
    B, Hkv, D = 1, 4, 128
    t = rtkv.DecodeTail(B, Hkv * D, torch.float16, "cpu", capacity=4)
    t.append(torch.zeros(B, 3, Hkv * D, dtype=torch.float16), torch.zeros(B, 3, Hkv * D, dtype=torch.float16))
    q = torch.zeros(B, Hkv, 3, D, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="ROCm"):
        rtkv.extend_attention(packed_stub(B, Hkv * D, torch.float16), q, Hkv, t)


def test_extend_module_rejects_masks_and_shapes():
    import rtkv
    B, Hq, Hkv, D, T = 1, 8, 4, 128, 3
    cache = rtkv.CompressedKVCache(B, 64, D)
    cache.store_packed(0, packed_stub(B, Hkv * D, torch.float16))
    att = rtkv.CompressedExtendAttention(cache, Hq, Hkv, D, 0)
    q = torch.zeros(B, Hq, T, D, dtype=torch.float16)
    kv = torch.zeros(B, Hkv, T, D, dtype=torch.float16)
    with pytest.raises(ValueError, match="mask"):
        att(q, kv, kv, attention_mask=torch.zeros(B, 1, T, T))
    with pytest.raises(ValueError):
        att(q, kv[:, :, :2], kv[:, :, :2])               # fewer keys than queries
    with pytest.raises(ValueError):
        att(q, kv, kv[:, :, :2])                         # K and V disagree
    with pytest.raises(ValueError):
        att(q[:, :4], kv, kv)                            # another head count
    with pytest.raises(ValueError):
        att(q[:, :, :, :64], kv[:, :, :, :64], kv[:, :, :, :64])   # another head_dim
    with pytest.raises(ValueError):
        att(q[:, :, :0], kv[:, :, :0], kv[:, :, :0])     # no token
    assert cache.tail_len(0) == 0                        # nothing was appended by the rejected calls
    with pytest.raises(RuntimeError, match="ROCm"):      # appends, then attention has no CPU path
        att(q, kv, kv)
    assert cache.tail_len(0) == T
    # the single-token module is as it was
    with pytest.raises(ValueError):
        rtkv.CompressedDecodeAttention(cache, Hq, Hkv, D, 0)(q[:, :, :2], kv[:, :, :2], kv[:, :, :2])
