"""End-to-end validation of the bench.py round flow (the driver contract).

Runs the REAL bench script under torchrun with world=2 on CPU/gloo
(--cpu-smoke): threaded co-resident opponents, deterministic per-opponent
consensus gather ordering across ranks, weak-scaling aggregate math.
This is the same code path the driver's 8-GPU RCCL run takes.
"""

import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_single_process_cpu_smoke():
    r = subprocess.run(
        [sys.executable, "bench.py", "--cpu-smoke", "--steps", "1",
         "--warmup", "0"],
        cwd=REPO, capture_output=True, text=True, timeout=300,
    )
    assert r.returncode == 0, r.stderr[-800:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["n_gpus"] == 1 and d["config"]["opponents"] == 3
    assert d["value"] > 0 and d["higher_is_better"] is True
    assert d["scaling"] == "weak"


def test_dump_outputs_cpu_smoke(tmp_path):
    """--dump-outputs writes the last timed round's gathered results as
    float32 arrays, identically for identical arguments; --full is
    accepted and leaves the result line's meaning unchanged."""
    import numpy as np

    def run(out_dir, *extra):
        r = subprocess.run(
            [sys.executable, "bench.py", "--cpu-smoke", "--steps", "2",
             "--warmup", "0", "--dump-outputs", str(out_dir), *extra],
            cwd=REPO, capture_output=True, text=True, timeout=300,
        )
        assert r.returncode == 0, r.stderr[-800:]
        d = json.loads(r.stdout.strip().splitlines()[-1])
        assert d["steps"] == 2 and d["ms_per_step"] > 0
        # value = critiques / elapsed, ms_per_step = elapsed / steps
        assert abs(d["value"] * d["ms_per_step"] / 1000.0
                   - d["config"]["opponents"]) < 1e-6
        return d, {p.stem: np.load(p) for p in sorted(out_dir.glob("*.npy"))}

    d, a = run(tmp_path / "a")
    assert set(a) == {"critique_tokens", "critique_lengths", "agreed",
                      "error", "all_agreed"}
    assert all(v.dtype == np.float32 for v in a.values())
    n, max_tok = d["config"]["opponents"], d["config"]["decode_tokens"]
    assert a["critique_tokens"].shape == (n, max_tok)
    assert a["critique_lengths"].shape == (n,)
    assert not a["error"].any()
    assert (a["critique_lengths"] <= max_tok).all()
    for row, ln in zip(a["critique_tokens"], a["critique_lengths"]):
        assert (row[: int(ln)] >= 0).all() and (row[int(ln):] == -1).all()

    d2, b = run(tmp_path / "b", "--full")
    assert d2["metric"] == d["metric"] and d2["unit"] == d["unit"]
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_torchrun_world2_gloo():
    env = dict(os.environ)
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29537", "bench.py", "--cpu-smoke",
         "--steps", "1", "--warmup", "0"],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=600,
    )
    assert r.returncode == 0, r.stderr[-800:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["n_gpus"] == 2
    assert d["config"]["opponents"] == 6  # weak scaling: 3 per rank
    assert d["config"]["parallelism"] == "opponent-parallel dp2"
