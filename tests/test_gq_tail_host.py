"""CPU: the argument checks of rtkv_gq_decode_attention_tail (one decode step over a layer in the rtkv-gq/1
format followed by a dense tail).  Every bad input below is refused on the host, before anything touches
a device — the pointers are made up — with RTKV_ERR_INVALID and a message that starts "rtkv: gq decode: ".
The good call they deviate from: H = 4 kv heads of 128, Hq = 8, fp16, row capacity 64, tail capacity 16."""
import ctypes

import pytest

INVALID = -1
FAKE = 1 << 20                                           # 16-byte aligned, never dereferenced

# bad input -> overrides of the good call
TABLE = {
    "null q":                   dict(q=0),
    "null tail struct":         dict(tail=None),
    "null rows_dev":            dict(rows_dev=0),
    "misaligned tail base":     dict(tail_k=FAKE + 8),
    "tail stride_s below Hkv*128": dict(stride_s=256),
    "negative tail capacity":   dict(tcap=-1),
    "workspace one byte short": dict(ws_short=1),
    "bad bit width":            dict(bits=(3, 4, 8)),
    "Hq % Hkv != 0":            dict(Hq=6),
    "two batch rows":           dict(B=2),
    "head_dim 64":              dict(D=64),
    "H not a multiple of 4":    dict(H=6),
}


def call(q=FAKE, tail="good", rows_dev=FAKE, tail_k=FAKE, stride_s=512, tcap=16, ws_short=0, bits=(2, 4, 8), Hq=8, B=1,
         D=128, H=4):
    import rtkv._lib as L
    from rtkv.group_quant import GqParams
    lib = L.lib()
    cap = 64
    kd = L.KVDesc()
    kd.k_dev, kd.v_dev, kd.dtype = FAKE, FAKE, L.F16
    kd.B, kd.S, kd.H, kd.D = B, 128, H, D
    kd.stride_b, kd.stride_s, kd.stride_h = 128 * H * D, H * D, D
    g = GqParams(4, 4, 4, 250)
    t = L.DenseTail(tail_k, FAKE, rows_dev, tcap, max(tcap, 1) * stride_s, stride_s) if tail == "good" else tail
    tp = ctypes.byref(t) if t is not None else None
    hq_ok = max(Hq - Hq % H, H)                          # the size function wants whole head groups
    n = lib.rtkv_gq_decode_tail_workspace_size(hq_ok, H, cap, max(tcap, 0))
    return lib.rtkv_gq_decode_attention_tail(ctypes.byref(kd), FAKE, FAKE, FAKE, (ctypes.c_int32 * 3)(*bits),
                                             ctypes.byref(g), FAKE, FAKE, FAKE, FAKE, 1 << 16, FAKE, FAKE, cap, q, Hq,
                                             0.1, tp, FAKE, FAKE, n - ws_short, None)


@pytest.mark.parametrize("bad", list(TABLE))
def test_bad_input_is_refused_on_the_host(bad):
    import rtkv._lib as L
    assert call(**TABLE[bad]) == INVALID, bad
    msg = L.lib().rtkv_last_error().decode()
    assert msg.startswith("rtkv: gq decode: "), (bad, msg)


def test_workspace_size_is_non_decreasing_in_both_capacities():
    import rtkv._lib as L
    size = L.lib().rtkv_gq_decode_tail_workspace_size
    caps = (0, 1, 63, 64, 65, 1000, 4096, 70000)
    for Hq, H in ((8, 4), (32, 32), (32, 8)):
        grid = [[size(Hq, H, rc, tc) for tc in caps] for rc in caps]
        for i in range(len(caps)):
            for j in range(len(caps)):
                assert grid[i][j] > 0
                if i:
                    assert grid[i][j] >= grid[i - 1][j], (Hq, H, caps[i], caps[j])
                if j:
                    assert grid[i][j] >= grid[i][j - 1], (Hq, H, caps[i], caps[j])
        # the list of sp + st partials of (2·Hkv + F) floats per query-head group
        assert size(Hq, H, 64, 64) == (Hq // H) * 2 * (2 * H + H * 128) * 4 + 256
