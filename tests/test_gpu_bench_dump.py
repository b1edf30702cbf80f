"""bench.py's plain run and --dump-outputs on a small workload (3 layers, S = 2048, 8 heads).

A plain run prints the headline fields only (nothing that needs --full); --dump-outputs writes the last
timed step's outputs as float32 / float64 .npy files that agree with each other, stay within the byte
budget, and come out the same from another process given the same arguments (seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--layers", "3", "--seq", "2048", "--heads", "8"]
FULL_ONLY = ("roofline", "roofline_path", "kernel_us_per_layer", "legs", "cpu_baseline")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")


def load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """(result line, dumped arrays) of one plain run in its own process."""
    d = str(tmp_path_factory.mktemp("dump"))
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *ARGS, "--dump-outputs", d],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), load(d)


@pytest.fixture(scope="module")
def job():
    """The same workload in this process, one step done."""
    import bench
    saved, sys.argv = sys.argv, ["bench.py", *ARGS]
    try:
        args = bench.resolve_config(bench.parse(), 1)
    finally:
        sys.argv = saved
    j = bench.Job(args, torch.device("cuda", 0), 0, 1)
    j.step()
    torch.cuda.synchronize()
    return j


def test_plain_line_has_the_headline_and_nothing_that_needs_full(plain):
    line, _ = plain
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "GB/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0 and line["value"] > 0 and isinstance(line["metric"], str)
    assert not [k for k in FULL_ONLY if k in line]


def test_dump_is_float_and_consistent(plain):
    _, a = plain
    n, S = 3, 2048
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64 * 10 ** 6
    assert a["layers"].tolist() == [0, 1, 2] and np.array_equal(a["tokens"], np.arange(S))
    for name in ("scores", "labels", "mask", "kept_index", "row_offset"):
        assert a[name].shape == (n, S), name
    assert a["scale_zp"].shape == (n, S, 4)
    assert np.isin(a["labels"], (0, 1, 2)).all() and np.isin(a["mask"], (0, 1)).all()
    assert np.isfinite(a["scores"]).all()
    for i in range(n):
        Sp = int(a["kept_rows"][i])
        assert 0 < Sp <= S
        assert np.array_equal(np.nonzero(a["mask"][i])[0], a["kept_index"][i, :Sp])
        assert (a["kept_index"][i, Sp:] == -1).all() and (a["row_offset"][i, Sp:] == -1).all()
        off = a["row_offset"][i, :Sp]  # one slot of the packed codes per kept row
        assert off.min() == 0 and np.unique(off).size == Sp and off.max() < a["packed_bytes"][i]
        assert (a["scale_zp"][i, Sp:] == 0).all() and np.isfinite(a["scale_zp"][i, :Sp]).all()
    for name in ("k_out_sample", "v_out_sample", "packed_k_sample", "packed_v_sample"):
        assert a[name].shape[0] == n and np.isfinite(a[name]).all(), name
    assert a["k_out_sample"].std() > 0.5  # K ~ N(0, 1) dequantized, not an untouched buffer
    pk = a["packed_k_sample"]
    assert pk.min() >= 0 and pk.max() <= 255 and np.array_equal(pk, np.round(pk))


def test_dump_is_the_same_from_another_process(plain, job, tmp_path):
    import bench
    _, a = plain
    bench.dump_outputs(job, str(tmp_path))
    b = load(str(tmp_path))
    assert sorted(a) == sorted(b)
    for name in a:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), name


def test_dump_reads_the_layer_buffers(job, tmp_path):
    """Whole arrays equal the buffers; a small budget samples the same positions of them."""
    import bench
    bench.dump_outputs(job, str(tmp_path / "whole"))
    w = load(str(tmp_path / "whole"))
    for l in range(3):
        assert np.array_equal(w["scores"][l], job.bufs[l].scores[0].cpu().numpy())
        assert np.array_equal(w["labels"][l], job.bufs[l].labels[0].cpu().numpy().astype(np.float32))
    budget = 200_000
    bench.dump_outputs(job, str(tmp_path / "small"), budget=budget)
    s = load(str(tmp_path / "small"))
    assert sum(x.nbytes for x in s.values()) <= budget
    tok = s["tokens"].astype(np.int64)
    assert 0 < tok.size < 2048 and (np.diff(tok) > 0).all()
    for name in ("scores", "labels", "mask", "kept_index", "row_offset", "scale_zp"):
        assert np.array_equal(s[name], w[name][:, tok]), name
    m = s["k_out_sample"].shape[1]
    assert 0 < m < w["k_out_sample"].shape[1]
    u = np.random.RandomState(20251019)
    u.choice(2048, tok.size, replace=False)
    u = u.random_sample(m)
    for l in range(3):
        pos = np.minimum((u * (w["kept_rows"][l] * job.F)).astype(np.int64), int(w["kept_rows"][l]) * job.F - 1)
        assert np.array_equal(s["k_out_sample"][l], job.bufs[l].k_out.cpu().numpy()[pos])
