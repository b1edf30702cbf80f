"""GPU: every kernel of the fused importance mode (csrc/qk_importance.hip, attn_lse.hip, attn_lse32.hip,
attn_f32.hip) against the float64 references, per-row bounds and exact count maps of tests/qk_checks.py, at
the edges of the kernels' own tiles.  Every case runs twice — random data (per-row bound, rows that see no key
exact) and zero keys (the count map: K1' bit for bit, the LSE within 4·2⁻²³·max(1, ln n)) — with 64 NaN
elements behind each output that must stay NaN.

Which case reaches which instantiation, read off the launchers (DT: float16 and bfloat16 alike):

  launch_qk_importance / launch_qk_dt — ring kernel when D < 128, or P ≤ 64, or S % 4 != 0 (and no key bias);
  nt = 2 (P ≤ 32), 4 (P ≤ 64), 8 (else), raised to 4 / ks when nt·ks < 4; ks = D / 32:
    qk_importance_kernel<DT, 4, 1>   test_ring[ring(4,1)-*]            D = 32, P ≤ 64
    qk_importance_kernel<DT, 8, 1>   test_ring[ring(8,1)-*]            D = 32, P > 64
    qk_importance_kernel<DT, 2, 2>   test_ring[ring(2,2)-*]            D = 64, P ≤ 32
    qk_importance_kernel<DT, 4, 2>   test_ring[ring(4,2)-*]            D = 64, 32 < P ≤ 64
    qk_importance_kernel<DT, 8, 2>   test_ring[ring(8,2)-*]            D = 64, P > 64
    qk_importance_kernel<DT, 2, 4>   test_ring[ring(2,4)-*]            D = 128, P ≤ 32
    qk_importance_kernel<DT, 4, 4>   test_ring[ring(4,4)-*]            D = 128, 32 < P ≤ 64
    qk_importance_kernel<DT, 8, 4>   test_ring[ring(8,4)-*]            D = 128, P > 64, S % 4 != 0;
                                     test_knobs[RTKV_QK_RING]          the same at S % 4 == 0
  launch_qk_head32 — D = 128, S % 4 == 0 and (P > 64 or a key bias); NTILE = the largest of 8, 4, 2, 1 with
  ceil(S / (128·NTILE))·H·B ≥ target (1024, 512 with a key bias, or RTKV_QK32_WGS):
    qk_head32_kernel<DT, false, 1, 2>   test_head32[*]                    (every S here gives far fewer workgroups)
    qk_head32_kernel<DT, true, 1, 3>    test_head32_key_padding[*]
    qk_head32_kernel<DT, *, 8, *>       test_knobs[RTKV_QK32_WGS=8]       S = 1028, H = 4: 2·4 = 8 ≥ 8;
                                                                          S = 132, H = 8: 1·8 ≥ 8
    qk_head32_kernel<DT, *, 4, *>       test_knobs[RTKV_QK32_WGS=12]      S = 1028, H = 4: 8 < 12 ≤ 3·4
    qk_head32_kernel<DT, *, 2, *>       test_knobs[RTKV_QK32_WGS=20]      S = 1028, H = 4: 12 < 20 ≤ 5·4
    (NTILE 4 without a knob: tests/test_gpu_qk.py's S = 16384 case.  At S = 132 NTILE 4 and 2 cannot be
    reached: ceil(132 / (128·NTILE)) = 1 for NTILE = 8, 4 and 2 alike, so the loop stops at 8 or falls to 1.)
  launch_qk_head:
    qk_head_kernel<DT, 8, 4>         test_knobs[RTKV_QK16]             rpw = 16: one 16-row tile per wave
                                     test_knobs[RTKV_QK16+RTKV_QK_WGS=1]   rpw = 256: 16 tiles per wave
  launch_qk_head_f32:
    qk_head_f32x3_kernel<16>         test_f32[*], test_f32_key_padding[*]
    qk_head_f32_kernel               test_knobs[RTKV_LSE_F32_EXACT]
  qk_head_reduce_kernel              every head-major case; all three head loops (32 + 8 + 3): test_reduce_43_heads
  launch_attention_lse:
    attn_lse32_kernel<DT> + attn_lse_kernel<DT, 4, 1> (fixup)   test_lse_*[float16-128*], [bfloat16-128*]; rows recomputed: test_lse_fixup
    attn_lse_kernel<DT, 2, 1>        test_lse_*[float16-64*], [bfloat16-64*]
    attn_lse_f32x3s_kernel<16>       test_lse_*[float32-128*]
    attn_lse_kernel<DT, 4, 1> as a full pass   test_knobs[RTKV_LSE_KERNEL=16]
    attn_lse_kernel<DT, 2, 2>        test_knobs[RTKV_LSE_RG=2]
    attn_lse_kernel<DT, 4, 2>        test_knobs[RTKV_LSE_RG=2+RTKV_LSE_KERNEL=16]
    (attn_lse_f32_kernel, the exact fp32 LSE: tests/test_gpu_lse.py.)

None of the instantiations named above is unreachable from the ABI; a kernel trace of every knob set's child and
of the default dispatch showed exactly the instantiations of this table.  S < P is reached as the sequence shards
reach it: the keys hold max(S, P) rows and the entry point reads the first P.

Measured on an MI355X, worst error/bound over each family's cases (float16 / bfloat16, or float32); no kernel
was found wrong, and the bound needed no further term:

  K1' ring (4,1) 0.072 / 0.062   (8,1) 0.033 / 0.030   (2,2) 0.032 / 0.031   (4,2) 0.026 / 0.022   (8,2) 0.023 / 0.020
           (2,4) 0.013 / 0.008   (4,4) 0.006 / 0.005   (8,4) 0.007 / 0.008   (8,4) at S % 4 == 0 (knob) 0.005 / 0.005
  K1' qk_head32_kernel 0.004 / 0.005, with a key bias 0.009 / 0.007, NTILE 8, 4, 2 (knob) 0.006 / 0.006 each
  K1' qk_head_kernel (knob) 0.009 / 0.007 at rpw = 16 and at rpw = 256
  K1' qk_head_f32x3_kernel 0.003, with a key bias 0.001; qk_head_f32_kernel (knob) 0.003; H = 43 0.001 / 0.0005 (fp32)
  K1' with row0 through the shard stage 0.005 / 0.009 / 0.001 (fp32)
  LSE attn_lse32_kernel + fix-up 0.013 / 0.014, key bias 0.012 / 0.013, overflowing rows 0.011 / 0.011
  LSE attn_lse_kernel<2, 1> 0.035 / 0.030, key bias 0.031 / 0.028; <2, 2> (knob) 0.035 / 0.030
  LSE attn_lse_kernel<4, 1> as a full pass and <4, 2> (knobs) 0.013 / 0.014
  LSE attn_lse_f32x3s_kernel 0.003 (key bias and overflowing rows alike)

Every K1' count map was exact, every LSE count map within 1.29 of the 4 allowed units of 2⁻²³·max(1, ln n), and
every guard region untouched.  (The ring kernels' ratios grow as D falls because the bound's leading term,
c_D·scale·T ∝ D^1.5, does: at D = 32 it is an eighth of what it is at D = 128 while exp2 and the sums cost the same.)

The knobs are read once per process, so each knob set runs in a child (tests/qk_knob_worker.py), one after
another under a time limit; the parent applies the checks.  A child that does not end cleanly fails its test and
the remaining knob tests are skipped: nothing more is started on a card after a fault."""
import json
import os
import subprocess
import sys

import pytest
import torch

import qk_checks as qc
from qk_checks import Case, case_id

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
HALF = ("float16", "bfloat16")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    import rtkv
    rtkv._lib.lib()


RATIOS = {}   # kernel family → worst error/bound seen (printed by the last test for the record)


def run_and_check(c, what, stages=None):
    r, ulps = qc.check_case(c, qc.run_case(c, stages=stages), what)
    key = (what, c.dtype)
    RATIOS[key] = (max(RATIOS.get(key, (0.0, 0.0))[0], r), max(RATIOS.get(key, (0.0, 0.0))[1], ulps))


# ---------------------------------------------------------------------------------------------- K1', ring
RING_S = (4, 61, 64, 65, 130, 257)
RING_P = {32: (1, 33, 64, 65, 128), 64: (1, 17, 32, 33, 63, 64, 65, 127, 128), 128: (1, 16, 32, 49, 64)}
HEADS3 = ((1, 1), (3, 3), (6, 2))


def ring_form(D, P):
    """launch_qk_dt's (NT, KS)."""
    ks = D // 32
    nt = 2 if P <= 32 else (4 if P <= 64 else 8)
    if nt * ks < 4:
        nt = 4 // ks
    return nt, ks


def _around(P, Ss):
    """The largest S below P, the smallest above it, and the largest of all."""
    below, above = [s for s in Ss if s < P], [s for s in Ss if s > P]
    return sorted(set(below[-1:] + above[:1] + [Ss[-1]]))


def _ring_cases():
    shapes = [(D, P, S) for D, Ps in RING_P.items() for P in Ps for S in _around(P, RING_S)]
    shapes += [(128, P, S) for P in (65, 127, 128) for S in (130, 257)]   # P > 64 stays here only if S % 4 != 0
    out = []
    for n, (D, P, S) in enumerate(shapes):
        H, Hkv = HEADS3[n % 3]
        for dt in HALF:
            out.append(Case(kind="k1", dtype=dt, B=2 if n % 4 == 1 else 1, H=H, Hkv=Hkv, S=S, D=D, P=P,
                            causal=n % 5 != 3))
    return out


RING = _ring_cases()
for _form in [(4, 1), (8, 1), (2, 2), (4, 2), (8, 2), (2, 4), (4, 4), (8, 4)]:
    for _dt in HALF:
        _hit = [c for c in RING if ring_form(c.D, c.P) == _form and c.dtype == _dt]
        assert any(c.B == 2 for c in _hit) and any(c.H != c.Hkv for c in _hit), _form
        assert _form == (8, 4) or any(c.S < c.P for c in _hit), _form   # (8, 4): S is 130 or 257 here
assert all(c.D < 128 or c.P <= 64 or c.S % 4 for c in RING)
assert {c.S for c in RING} == set(RING_S)


@pytest.mark.parametrize("c", RING, ids=lambda c: "ring(%d,%d)-" % ring_form(c.D, c.P) + case_id(c))
def test_ring(c):
    run_and_check(c, "ring(%d,%d)" % ring_form(c.D, c.P))


# ------------------------------------------------------------------------------------ K1', qk_head32_kernel
HEAD32_PS = {65: (68, 256, 1028), 96: (68, 128, 260), 97: (68, 128, 132), 127: (68, 128, 256),
             128: (68, 128, 132, 260, 1028)}
HEAD32 = [Case(kind="k1", dtype=dt, B=2 if n % 3 == 1 else 1, H=8, Hkv=2, S=S, D=128, P=P, causal=n % 5 != 2)
          for n, (P, S) in enumerate((P, S) for P, Ss in HEAD32_PS.items() for S in Ss) for dt in HALF]
assert {c.S for c in HEAD32} == {68, 128, 132, 256, 260, 1028} and all(c.S % 4 == 0 and c.P > 64 for c in HEAD32)


def pads(S, left, B=2):
    """Batch row 0: `left` leading padding keys; the last batch row: trailing padding from one row before a 32-row
    tile edge."""
    first = 32 * ((S - 1) // 32) - 1
    first = first if first >= 1 else S - 1
    if B == 1:
        return ((left,), (0,))
    return ((left, 0), (0, S - first))


# left padding that ends inside the prompt (5; 1 for P = 1 would leave nothing: there the whole prompt is
# padding and every live row's A is exactly 0), on a 32-row tile edge and one row past it
KB_CASES = [(P, S, left) for P in (1, 26, 97, 128) for S, left in ((132, 5), (260, 32), (132, 33))]
HEAD32_KB = [Case(kind="k1", dtype=dt, B=2, H=8, Hkv=2, S=S, D=128, P=P, pad=pads(S, left))
             for P, S, left in KB_CASES for dt in HALF]


@pytest.mark.parametrize("c", HEAD32, ids=case_id)
def test_head32(c):
    run_and_check(c, "head32")


@pytest.mark.parametrize("c", HEAD32_KB, ids=case_id)
def test_head32_key_padding(c):
    run_and_check(c, "head32 KB")


# ------------------------------------------------------------------------------------------- K1', float32
F32_PS = {1: (4, 255, 516), 17: (16, 255, 260), 64: (16, 255, 256), 97: (16, 255, 516), 128: (4, 255, 256, 260, 516)}
F32 = [Case(kind="k1", dtype="float32", B=2 if n % 3 == 1 else 1, H=HEADS3[n % 3][0], Hkv=HEADS3[n % 3][1], S=S, D=128,
            P=P, causal=n % 5 != 2) for n, (P, S) in enumerate((P, S) for P, Ss in F32_PS.items() for S in Ss)]
F32_KB = [Case(kind="k1", dtype="float32", B=2, H=6, Hkv=2, S=S, D=128, P=P, pad=pads(S, left))
          for P, S, left in ((1, 16, 5), (17, 256, 5), (64, 260, 32), (97, 516, 33), (128, 260, 33), (128, 516, 5))]


@pytest.mark.parametrize("c", F32, ids=case_id)
def test_f32(c):
    run_and_check(c, "f32x3")


@pytest.mark.parametrize("c", F32_KB, ids=case_id)
def test_f32_key_padding(c):
    run_and_check(c, "f32x3 KB")


@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_reduce_43_heads(dtype):
    """H = 43 = 32 + 8 + 3: qk_head_reduce_kernel's three head loops in one sum."""
    run_and_check(Case(kind="k1", dtype=dtype, B=2, H=43, Hkv=43, S=132, D=128, P=97), "reduce H=43")


# ------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("c", [
    Case(kind="k1", dtype="bfloat16", B=2, H=6, Hkv=2, S=65, D=64, P=33),        # ring
    Case(kind="k1", dtype="float16", B=2, H=8, Hkv=2, S=132, D=128, P=97),       # head32
    Case(kind="k1", dtype="float32", B=2, H=6, Hkv=2, S=260, D=128, P=97),       # f32x3
], ids=case_id)
def test_layouts_are_bit_equal(c):
    """Keys as [B, Hkv, S, D], and Q as the transposed view of a [B, S, H, D] tensor (q_stride_s = H·D, what a
    model's projection gives before .contiguous()): bit-equal to the contiguous result."""
    inp, lse_in = qc.inputs(c), qc.lse_reference(c, with_bound=False).lse_in
    A = qc.run_k1(c, inp, lse_in)
    qc.check_A(A, c, "layout bsf")
    assert torch.equal(qc.run_k1(c, inp, lse_in, layout="bhsd"), A)
    assert torch.equal(qc.run_k1(c, inp, lse_in, layout="q_bshd"), A)


# --------------------------------------------------------------------------------------------------- row0
ROW0 = [(128, r) for r in (1, 37, 63, 64, 100, 127, 128)] + [(60, 59), (60, 60)]
SHARD = [Case(kind="k1", dtype=dt, B=2 if n % 2 else 1, H=4, Hkv=2, S=S, D=D, P=P, row0=r)
         for n, (P, r) in enumerate(ROW0) for S in (64, 132) for dt, D in (("float16", 128), ("bfloat16", 64),
                                                                          ("float32", 128))]


@pytest.mark.parametrize("c", SHARD, ids=case_id)
def test_row0_through_the_shard_stage(c):
    """The causal edge inside the prompt with row0 > 0, through HipShardStages.aggregate_qk (prompt keys [B, P, F]
    as rank 0 broadcasts them, the rank's own query rows and lse)."""
    from rtkv.sharded import HipShardStages
    run_and_check(c, "row0", stages=HipShardStages("cuda"))


# ---------------------------------------------------------------------------------------------------- LSE
LSE_KERNELS = (("float16", 128), ("bfloat16", 128), ("float16", 64), ("bfloat16", 64), ("float32", 128))
LSE_S = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 193, 255, 256, 257, 300)
LSE_NAME = {128: "lse32+fixup", 64: "lse<2,1>"}


def lse_name(dt, D):
    return "lse f32x3s" if dt == "float32" else LSE_NAME[D]


def lse_sweep(dt, D, causal):
    # H = 2, B = 2: nblk·H·B is a multiple of 8 where nblk is even and not where it is odd — both branches of
    # the workgroup remap, at every kernel's own block size
    return [Case(kind="lse", dtype=dt, B=2, H=2, Hkv=2, S=S, D=D, causal=causal) for S in LSE_S]


def lse_random(dt, D):
    # 8/2: nblk·8 is always a multiple of 8; 6/2 with an odd nblk is not
    return [Case(kind="lse", dtype=dt, B=B, H=H, Hkv=2, S=S, D=D, causal=causal)
            for S in (65, 129, 257, 300) for H, B, causal in ((8, 1, True), (6, 1, S != 129))] + \
           [Case(kind="lse", dtype=dt, B=2, H=8, Hkv=2, S=300, D=D)]


def lse_padded(dt, D):
    return [Case(kind="lse", dtype=dt, B=2, H=4, Hkv=2, S=S, D=D, pad=pads(S, left))
            for S, left in ((132, 5), (260, 32), (132, 33), (260, 64), (300, 65))]


BOOST_KEY = 70   # in the second 64-key tile: lane 6 of attn_lse32_kernel has taken key 6 or 38 as its reference by then


def lse_overflow(dt, D):
    """Rows whose logit at key 70 is ~260 log2 units above the one their lane took as its reference in the first key
    tile: the 32x32 kernel's unchecked sum overflows and the fix-up recomputes their 64-row block.  Under a causal
    mask rows 0 .. 63 see the first tile only, so the first block overflows in the full-attention case: rows 10 ..
    20 of it (beside valid rows), all of block 2 (alone in it) and rows of the partial last block (S = 300).
    Causal: block 1, whose rows 64 .. 69 do not see the key (valid rows beside overflowing ones), all of block 3,
    the partial block; and S = 128, B = 2: the last full block."""
    k = BOOST_KEY
    return [Case(kind="lse", dtype=dt, B=1, H=2, Hkv=2, S=300, D=D, causal=False, boost=(k, ((10, 20), (128, 191), (290, 299)))),
            Case(kind="lse", dtype=dt, B=1, H=2, Hkv=2, S=300, D=D, boost=(k, ((64, 127), (192, 255), (290, 299)))),
            Case(kind="lse", dtype=dt, B=2, H=2, Hkv=1, S=128, D=D, boost=(k, ((64, 127),)))]


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("dt,D", LSE_KERNELS, ids=lambda v: str(v))
def test_lse_lengths(dt, D, causal):
    for c in lse_sweep(dt, D, causal):
        run_and_check(c, lse_name(dt, D))


@pytest.mark.parametrize("dt,D", LSE_KERNELS, ids=lambda v: str(v))
def test_lse_random(dt, D):
    for c in lse_random(dt, D):
        run_and_check(c, lse_name(dt, D))


@pytest.mark.parametrize("dt,D", LSE_KERNELS, ids=lambda v: str(v))
def test_lse_key_padding(dt, D):
    for c in lse_padded(dt, D):
        run_and_check(c, lse_name(dt, D) + " KB")


@pytest.mark.parametrize("dt,D", LSE_KERNELS, ids=lambda v: str(v))
def test_lse_fixup(dt, D):
    for c in lse_overflow(dt, D):
        key, rows = c.boost
        x = qc.logits(c, qc.inputs(c), 0).x * 1.4426950408889634          # [H, S, S] in log2 units
        for a, z in rows:   # the rows are what the case says: the boosted key is more than 128 above the reference
            a = a if not c.causal else max(a, key)
            first = torch.maximum(x[:, a:z + 1, key % 32], x[:, a:z + 1, key % 32 + 32])
            assert float((x[:, a:z + 1, key] - first).min()) > 128.0
        run_and_check(c, lse_name(dt, D) + " overflow")


# -------------------------------------------------------------------------------------------------- knobs
def lse_all(D):
    return [c for dt in HALF for causal in (True, False) for c in lse_sweep(dt, D, causal)] + \
           [c for dt in HALF for f in (lse_random, lse_padded, lse_overflow) for c in f(dt, D)]


# RTKV_QK32_WGS = target in launch_qk_head32's loop `nt = 8; while (nt > 1 && wgs(nt) < target) nt /= 2`, with
# wgs(nt) = ceil(S / (128·nt))·H·B.  S = 1028, H = 4, B = 1: wgs(8) = 2·4 = 8, wgs(4) = 3·4 = 12, wgs(2) = 5·4 = 20,
# wgs(1) = 36, so target 8 → NTILE 8, 12 → 4, 20 → 2 (a key bias changes the default target only, not the
# knob).  The last workgroup of each starts at row 1024: one tile with 4 rows below S, the rest wholly past S.
# S = 132, H = 8: wgs(8) = wgs(4) = wgs(2) = 8, wgs(1) = 16: NTILE 8 at target 8 (rows 132 .. 1023 of the one
# workgroup wholly past S), NTILE 1 at the two others.
WGS = [Case(kind="k1", dtype=dt, B=1, H=H, Hkv=2, S=S, D=128, P=P, pad=pad)
       for dt in HALF for S, H in ((1028, 4), (132, 8)) for P in (97, 128)
       for pad in (None, pads(S, 33, B=1))]

KNOBS = [
    ("RTKV_QK_RING", {"RTKV_QK_RING": "1"}, HEAD32, "ring(8,4) S%4=0"),
    ("RTKV_QK16", {"RTKV_QK16": "1"}, HEAD32 + HEAD32_KB, "head16"),
    ("RTKV_QK16+RTKV_QK_WGS=1", {"RTKV_QK16": "1", "RTKV_QK_WGS": "1"}, HEAD32 + HEAD32_KB, "head16 rpw=256"),
    ("RTKV_QK32_WGS=8", {"RTKV_QK32_WGS": "8"}, WGS, "head32 NTILE=8"),
    ("RTKV_QK32_WGS=12", {"RTKV_QK32_WGS": "12"}, WGS, "head32 NTILE=4"),
    ("RTKV_QK32_WGS=20", {"RTKV_QK32_WGS": "20"}, WGS, "head32 NTILE=2"),
    ("RTKV_LSE_KERNEL=16", {"RTKV_LSE_KERNEL": "16"}, lse_all(128), "lse<4,1> full"),
    ("RTKV_LSE_RG=2", {"RTKV_LSE_RG": "2"}, lse_all(64), "lse<2,2>"),
    ("RTKV_LSE_RG=2+RTKV_LSE_KERNEL=16", {"RTKV_LSE_RG": "2", "RTKV_LSE_KERNEL": "16"}, lse_all(128), "lse<4,2>"),
    ("RTKV_LSE_F32_EXACT", {"RTKV_LSE_F32_EXACT": "1"}, F32 + F32_KB, "f32 exact"),
]
ALL_KNOBS = ("RTKV_QK_RING", "RTKV_QK16", "RTKV_QK_WGS", "RTKV_QK32_WGS", "RTKV_LSE_KERNEL", "RTKV_LSE_RG",
             "RTKV_LSE_F32_EXACT")
CHILD_SECONDS = 90    # torch import and device start-up (most of it), then a few seconds of tiny launches
_child_failed = []    # a child that did not end cleanly: no further child is started


@pytest.mark.parametrize("name,env,cases,what", KNOBS, ids=[k[0] for k in KNOBS])
def test_knobs(name, env, cases, what, tmp_path):
    if _child_failed:
        pytest.skip(f"the {_child_failed[0]} child did not end cleanly: nothing more is started on the card")
    spec, out = tmp_path / "cases.json", tmp_path / "out.pt"
    spec.write_text(json.dumps([list(c) for c in cases]))
    child_env = {k: v for k, v in os.environ.items() if k not in ALL_KNOBS}
    child_env.update(env)
    try:
        p = subprocess.run([sys.executable, "-u", os.path.join(HERE, "qk_knob_worker.py"), str(spec), str(out)],
                           env=child_env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=CHILD_SECONDS)
    except subprocess.TimeoutExpired as e:
        _child_failed.append(name)
        pytest.fail(f"{name}: the child did not end within {CHILD_SECONDS} s:\n{(e.stdout or '')[-4000:]}")
    if p.returncode != 0 or "worker ok" not in p.stdout:
        _child_failed.append(name)
        pytest.fail(f"{name}: the child ended with {p.returncode}:\n{p.stdout[-4000:]}")
    d = torch.load(out, weights_only=True)
    assert [qc.freeze(c) for c in d["cases"]] == list(cases)
    for c, outs in zip(cases, d["outs"]):
        r, ulps = qc.check_case(c, outs, what)
        key = (what, c.dtype)
        RATIOS[key] = (max(RATIOS.get(key, (0.0, 0.0))[0], r), max(RATIOS.get(key, (0.0, 0.0))[1], ulps))


def test_zz_print_worst_ratios():
    """For the record (pytest -s): per kernel family and dtype, the worst error/bound of this run and the worst
    count-map error of the LSE in units of 2⁻²³·max(1, ln n) (K1's count maps are exact or the test failed)."""
    for (what, dt), (r, ulps) in sorted(RATIOS.items()):
        print(f"WORST {what:24s} {dt:9s} error/bound {r:.4f}  count map {ulps:.2f} ulp")
