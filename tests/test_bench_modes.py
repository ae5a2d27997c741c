"""bench.py's two modes: a plain run does only the headline measurement (and, for --dump-outputs, one untimed decode of the last step's
files); --full adds the other legs.  Both write the same arrays for --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.support import ROOT
FULL_ONLY = ("sweep", "config4_per_gpu_shape", "host_path", "decode", "cpu_baseline")


def _bench(*extra):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "64", "--steps", "2", "--warmup", "1", *extra],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-1500:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_what_a_full_run_dumps(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    assert plain["value"] > 0 and plain["unit"] == "Mpixels/s" and plain["higher_is_better"] is True and plain["dtype"] == "int16"
    assert plain["ms_per_step"] > 0 and plain["images_ok"] == [64]
    assert not any(k in plain for k in FULL_ONLY), sorted(plain)
    assert "hbm_copy_measured" not in plain["roofline"] and "chroma_l1_ms" not in plain["roofline"] and not plain["roofline"]["chroma_l1_in_frac"]

    # every leg but the slow ones: the decode leg is the one whose last timed step the dump holds
    full = _bench("--full", "--sweep=", "--no-cpu-baseline", "--no-host-path", "--no-config4-shape", "--dump-outputs", str(tmp_path / "full"))
    assert full["decode"]["files_ok_rank0"] == 64 and full["roofline"]["hbm_copy_measured"] > 0 and full["roofline"]["chroma_l1_in_frac"]
    assert plain["bytes_out"] == full["bytes_out"]

    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full")) and "dec_pixels_sha52.npy" in names and "enc_nhw_sha52.npy" in names
    for n in names:
        a, b = np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)
        assert a.dtype == b.dtype and np.array_equal(a, b), n
