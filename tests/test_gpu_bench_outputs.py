"""bench.py --dump-outputs and --full.  --dump-outputs DIR writes what the last timed step computed (train: the three losses and every
network's parameters after the update; eval: the four embedding matrices) as float32 / float64 .npy files, at most 64 MB in all, and
two runs with the same arguments write the same arrays (seeded inputs, the train step in deterministic mode).  A plain line carries the
headline figures only; --full adds the roofline and the CPU baseline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = ["net_video_local", "net_video_global", "net_text_local", "net_text_global"]


def _bench(*args, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    out = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values()), {k: a.dtype for k, a in out.items()}
    assert sum(a.nbytes for a in out.values()) <= 64e6
    assert all(np.isfinite(a).all() for a in out.values())
    return out


@pytest.mark.timeout(600)
def test_dump_outputs_of_the_train_step_are_the_same_every_run(tmp_path):
    dumps = []
    for r in range(2):
        d = _bench("--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / f"run{r}"))
        assert d["steps"] == 2 and d["ms_per_step"] > 0 and "roofline" not in d and "cpu_baseline" not in d
        dumps.append(_load(str(tmp_path / f"run{r}")))
    a, b = dumps
    assert sorted(a) == sorted(["losses"] + [f"params_{n}" for n in NETS])
    assert a["losses"].dtype == np.float64 and a["losses"].shape == (3,)
    assert abs(a["losses"][0] - a["losses"][1] - a["losses"][2]) <= 1e-6 * abs(a["losses"][0])  # total = contrastive + cycle-consistency
    assert all(a[f"params_{n}"].dtype == np.float32 and a[f"params_{n}"].ndim == 1 for n in NETS)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.timeout(300)
def test_dump_outputs_of_the_eval_forward(tmp_path):
    _bench("--steps", "2", "--warmup", "1", "--eval", "--dump-outputs", str(tmp_path))
    e = _load(str(tmp_path))
    assert sorted(e) == ["clip_emb", "par_emb", "sent_emb", "vid_emb"]
    assert e["vid_emb"].shape == (64, 768) and e["clip_emb"].shape == (256, 384)


@pytest.mark.timeout(600)
def test_full_adds_roofline_and_cpu_baseline():
    d = _bench("--steps", "2", "--warmup", "1", "--full")
    assert d["roofline"]["unit"] == "TFLOP/s" and d["roofline"]["achieved"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["unit"] == "clip-pairs/s"
