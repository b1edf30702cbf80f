"""CPU: the argument checks shared by the three attention entry points over the packed cache
(rtkv_decode_attention_packed, rtkv_decode_attention_packed_tail, rtkv_extend_attention_packed_tail).
Every bad input below is refused on the host, before anything touches a device — the pointers are made
up — with the entry point's status code and a message that starts with its prefix.  The multi-token
step reports what lies outside its kernel's envelope (Hkv*D, field widths) as RTKV_ERR_UNSUPPORTED,
the decode step everything as RTKV_ERR_INVALID."""
import ctypes

import pytest

INVALID, UNSUPPORTED = -1, -2
FAKE = 1 << 20                                           # 16-byte aligned, never dereferenced
ENTRIES = ("decode", "decode_tail", "extend")

# bad input -> (overrides of the good call, status per entry point; None: the entry point has no such argument)
TABLE = {
    "null q":                   (dict(q=0), (INVALID, INVALID, INVALID)),
    "null tail struct":         (dict(tail=None), (None, INVALID, INVALID)),
    "Hq % Hkv != 0":            (dict(Hq=6), (INVALID, INVALID, INVALID)),
    "Hkv*D not a multiple of 512": (dict(Hkv=2), (INVALID, INVALID, UNSUPPORTED)),
    "misaligned q":             (dict(q=FAKE + 8), (INVALID, INVALID, INVALID)),
    "tail stride_s below Hkv*D": (dict(stride_s=256), (None, INVALID, INVALID)),
    "workspace one byte short": (dict(ws_short=1), (INVALID, INVALID, INVALID)),
    "bad bit width":            (dict(bits=(3, 4, 8)), (INVALID, INVALID, UNSUPPORTED)),
    "null packed pointer":      (dict(row_offset=0), (INVALID, INVALID, INVALID)),
}


def call(entry, q=FAKE, tail="good", Hq=8, Hkv=4, stride_s=512, ws_short=0, bits=(2, 4, 8), row_offset=FAKE):
    """One call with a packed layer of 64 rows' capacity, a tail of 16, fp16, head_dim 128, T = 4."""
    import rtkv._lib as L
    lib = L.lib()
    D, cap, tcap, T = 128, 64, 16, 4
    packed = (FAKE, FAKE, 1 << 16, row_offset, FAKE, FAKE, FAKE, 1, 128, cap, FAKE, Hkv, D, L.F16,
              (ctypes.c_int32 * 3)(*bits))
    t = L.DenseTail(FAKE, FAKE, FAKE, tcap, tcap * stride_s, stride_s) if tail == "good" else tail
    tp = ctypes.byref(t) if t is not None else None
    hq_ok = Hq - Hq % Hkv                                # the size functions want whole head groups
    if entry == "decode":
        n = lib.rtkv_decode_workspace_size(1, hq_ok, Hkv, D, cap)
        return lib.rtkv_decode_attention_packed(*packed, q, Hq, 0.1, FAKE, FAKE, n - ws_short, None)
    if entry == "decode_tail":
        n = lib.rtkv_decode_tail_workspace_size(1, hq_ok, Hkv, D, cap, tcap)
        return lib.rtkv_decode_attention_packed_tail(*packed, q, Hq, 0.1, tp, FAKE, FAKE, n - ws_short, None)
    n = lib.rtkv_extend_workspace_size(1, hq_ok, Hkv, D, T, cap, tcap)
    return lib.rtkv_extend_attention_packed_tail(*packed, q, Hq * T * D, T * D, D, Hq, T, 0.1, tp, FAKE, FAKE,
                                                 n - ws_short, None)


@pytest.mark.parametrize("bad", list(TABLE))
def test_bad_input_is_refused_alike_by_all_entry_points(bad):
    import rtkv._lib as L
    overrides, statuses = TABLE[bad]
    for entry, want in zip(ENTRIES, statuses):
        if want is None:
            continue
        assert call(entry, **overrides) == want, (bad, entry)
        msg = L.lib().rtkv_last_error().decode()
        assert msg.startswith("rtkv: " + ("extend: " if entry == "extend" else "decode: ")), (bad, entry, msg)
