"""CPU-only: bench.py's own launcher (python bench.py --gpus N without torch.distributed.run)."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(torch.cuda.device_count() >= 2, reason="this node could run the two ranks")
def test_more_ranks_than_devices_is_one_error_line_not_a_launch():
    """The round-3 review: `python3 bench.py --gpus N` with no WORLD_SIZE must start by itself, and a failure must be a JSON error
    line with rc != 0, never a hang.  With fewer devices than ranks nothing is launched at all."""
    cp = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"], capture_output=True,
                        text=True, timeout=300, env={k: v for k, v in os.environ.items() if k != "WORLD_SIZE"})
    assert cp.returncode == 2, (cp.returncode, cp.stderr[-500:])
    line = json.loads(cp.stdout.strip().splitlines()[-1])
    assert "error" in line and line["n_gpus"] == 2


def test_dump_outputs_writes_the_table_and_samples_above_the_limit(tmp_path):
    """`--dump-outputs`: the arrays give the table back row for row; a table above the size limit is cut to the same sample of
    its rows on every run, and the files stay within the limit."""
    import numpy as np

    import bench

    names = ["F%d" % i for i in range(50)]
    table = [([names[(7 * r + k) % 50] for k in range(1 + r % 5)], 3 * r + 1) for r in range(400)]

    def load(d):
        a = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
        assert sorted(a) == ["callset_features", "callset_offsets", "counts", "row_index"]
        assert all(v.dtype == np.float64 for v in a.values())
        off = a["callset_offsets"].astype(int)
        rows = [([names[int(p)] for p in a["callset_features"][off[i]:off[i + 1]]], int(c)) for i, c in enumerate(a["counts"])]
        return a["row_index"].astype(int).tolist(), rows

    bench.dump_outputs(str(tmp_path / "all"), table, names)
    index, rows = load(str(tmp_path / "all"))
    assert index == list(range(400)) and rows == table

    for d in ("cut", "again"):
        bench.dump_outputs(str(tmp_path / d), table, names, limit=4096)
    index, rows = load(str(tmp_path / "cut"))
    assert 0 < len(index) < 400 and index == sorted(set(index)) and rows == [table[i] for i in index]
    assert load(str(tmp_path / "again")) == (index, rows)
    assert sum(os.path.getsize(str(tmp_path / "cut" / f)) for f in os.listdir(str(tmp_path / "cut"))) <= 4096
