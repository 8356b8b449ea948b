"""bench.py's stdout contract: the driver reads ONE JSON line.  Native libraries (RCCL's version banner at
communicator init) write to file descriptor 1; bench.quiet_native_stdout() points fd 1 at stderr and
bench.emit() writes the line to a duplicate of the original stdout."""
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_one_json_line_despite_native_stdout_writes():
    code = (
        "import os, sys\n"
        f"sys.path.insert(0, {str(ROOT)!r})\n"
        "import bench\n"
        "bench.quiet_native_stdout()\n"
        "os.write(1, b'RCCL version : banner on fd 1\\n')\n"
        "print('python print after the redirect')\n"
        "bench.emit({'metric': 'm', 'value': 1.0})\n"
    )
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    assert json.loads(lines[0]) == {"metric": "m", "value": 1.0}
    assert "RCCL version" in r.stderr and "python print" in r.stderr


def test_dump_outputs_keeps_small_outputs_whole_and_samples_large_ones_alike(tmp_path, monkeypatch):
    """--dump-outputs: float64 files; an output within the size limit is written whole; a larger one as the
    same sorted sample of rows for each of its columns, the same in every run, all files within the limit."""
    import numpy as np
    import torch

    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 3 * 4096 + 3 * 8 * 1000)   # three columns of 1000 rows
    keys = torch.arange(5000, dtype=torch.int64) * 3 + 7
    sums = keys * 1000 + 1
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, {"vertex": keys, "sum": sums}, {"count": 42})
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["count.npy", "sum.npy", "vertex.npy"]
    k, s, c = (np.load(tmp_path / "a" / f"{n}.npy") for n in ("vertex", "sum", "count"))
    assert k.dtype == s.dtype == c.dtype == np.float64 and c.tolist() == [42.0]
    assert k.shape == s.shape == (1000,) and np.all(np.diff(k) > 0)
    assert np.array_equal(s, k * 1000 + 1) and np.all((k - 7) % 3 == 0)   # rows of the output, columns aligned
    assert all(np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)) for f in files)
    assert sum((tmp_path / "a" / f).stat().st_size for f in files) <= bench.DUMP_BYTES
