"""bench.py --dump-outputs: the arrays of the timed path's last step as .npy
(float32 / float64), identical from run to run, bounded in size; and the
plain line carries the headline figure only (`--full` holds the rest)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
W, N, STEPS = 96, 60, 3
NAMES = ("sequences", "scores", "counters", "walker_ids")


def _load(d, suffix=""):
    return {k: np.load(os.path.join(d, k + suffix + ".npy")) for k in NAMES}


def test_write_outputs_layout_and_bounded_sample(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench

    rng = np.random.default_rng(5)
    seqs = ["".join(rng.choice(list("ACGU"), size=N)) for _ in range(W)]
    scores = rng.standard_normal(W)
    counters = rng.integers(0, 9, size=(W, 4)).astype(np.int64)
    gids = list(range(7, 7 + W))

    bench.write_outputs(str(tmp_path / "all"), 0, 1, gids, seqs, scores, counters)
    z = _load(tmp_path / "all")
    assert z["sequences"].dtype == np.float32 and z["sequences"].shape == (W, N)
    assert all(z[k].dtype == np.float64 for k in ("scores", "counters", "walker_ids"))
    assert ["".join(chr(int(c)) for c in row) for row in z["sequences"]] == seqs
    assert np.array_equal(z["scores"], scores) and np.array_equal(z["counters"], counters)
    assert np.array_equal(z["walker_ids"], gids)

    # over the size bound: a fixed sample of the walkers, the same on every call, each
    # rank holding its share of the bound under its own file names
    per_walker = 4 * N + 8 * 6
    monkeypatch.setattr(bench, "DUMP_BYTES", 2 * 10 * per_walker)
    for d in ("s1", "s2"):
        bench.write_outputs(str(tmp_path / d), 1, 2, gids, seqs, scores, counters)
    a, b = _load(tmp_path / "s1", "_rank1"), _load(tmp_path / "s2", "_rank1")
    assert all(np.array_equal(a[k], b[k]) for k in NAMES)
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BYTES // 2
    rows = (a["walker_ids"] - 7).astype(int)
    assert len(rows) == 10 and len(set(rows)) == 10 and list(rows) == sorted(rows)
    assert np.array_equal(a["scores"], scores[rows]) and np.array_equal(a["counters"], counters[rows])
    assert ["".join(chr(int(c)) for c in row) for row in a["sequences"]] == [seqs[r] for r in rows]


def _bench(args):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--walkers", str(W), "--length", str(N)] + args,
                       capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_reproducibly(tmp_path):
    args = ["--steps", str(STEPS), "--warmup", "1"]
    out = _bench(args + ["--dump-outputs", str(tmp_path / "a"), "--dump-walkers", str(tmp_path / "w")])
    _bench(args + ["--dump-outputs", str(tmp_path / "b")])
    # the plain line: the headline figure, none of what --full measures
    assert out["steps"] == STEPS and out["value"] > 0 and out["higher_is_better"] and out["dtype"] == "i16x2"
    assert out["value"] == pytest.approx(W * 1e3 / out["ms_per_step"], rel=1e-9)
    assert not {"roofline", "cpu_baseline", "sub_records"} & set(out)
    assert sum(out["config"]["outcomes"].values()) == W * STEPS   # --steps is the number of timed steps
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(os.listdir(tmp_path / "a")) == sorted(k + ".npy" for k in NAMES)
    assert a["sequences"].dtype == np.float32 and a["sequences"].shape == (W, N)
    assert a["scores"].dtype == a["counters"].dtype == np.float64
    # (a score may be -inf: an MFE fold that satisfies "active" makes apo's "not active" log 0)
    assert not np.isnan(a["scores"]).any()
    for k in NAMES:   # same arguments, same inputs: the same outputs bit for bit
        assert np.array_equal(a[k], b[k]), k
    # and they are the walkers the engine holds after the last timed step
    z = np.load(os.path.join(tmp_path / "w", "rank0.npz"))
    assert ["".join(chr(int(c)) for c in row) for row in a["sequences"]] == [str(s) for s in z["seqs"]]
    assert np.array_equal(a["scores"], z["scores"]) and np.array_equal(a["counters"], z["counters"])
    assert a["counters"].sum() == W * (STEPS + 1)   # warm-up step included
