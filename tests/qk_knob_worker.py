"""One child process of tests/test_gpu_qk_variants.py's knob tests (run as its own process; not collected by
pytest).

    python tests/qk_knob_worker.py CASES.json OUT.pt

The fused importance mode reads its cross-check knobs (RTKV_QK_RING, RTKV_QK16, RTKV_QK_WGS, RTKV_QK32_WGS,
RTKV_LSE_KERNEL, RTKV_LSE_RG, RTKV_LSE_F32_EXACT) once per process, so each knob set gets a process of its own
with the knobs in its environment.  The child reads the case list (qk_checks.Case tuples as JSON), draws the
same synth inputs as the parent, runs the library on each case's random data and count map (qk_checks.run_case)
and saves the outputs; the parent applies the float64 bound and the count map."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "golden"), os.path.join(HERE, "..", "realtime-kv-cache-compression_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    import qk_checks as qc
    import rtkv
    with open(sys.argv[1]) as f:
        cases = [qc.freeze(c) for c in json.load(f)]
    rtkv._lib.lib()
    assert torch.cuda.is_available()
    outs = [qc.run_case(c) for c in cases]
    torch.save({"cases": [list(c) for c in cases], "outs": outs}, sys.argv[2])
    print(f"worker ok: {len(cases)} cases")


if __name__ == "__main__":
    main()
