"""bench.py on the device: a plain run times exactly --steps steps and prints the headline line alone (no --full objects), and
--dump-outputs writes what the timed pass computed -- equal to the same pass over the same device-generated batch here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_and_its_dumped_outputs(tmp_path):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 4 and d["warmup"] == 2 and d["full"] is False
    assert d["unit"] == "passes/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["timing"]["repeats"] == 1 and d["ms_per_step"] > 0
    assert abs(d["value"] - 1024 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["device"] is None and "secondary" not in d

    info = d["outputs"]
    assert info["files"] == ["P_smooth", "f_smooth", "loglik"] and info["of_replicates"] == 1024
    got = {n: np.load(out / f"{n}.npy") for n in info["files"]}
    assert all(x.dtype == np.float64 for x in got.values())
    assert sum(os.path.getsize(out / f"{n}.npy") for n in info["files"]) <= 64 * 10**6
    S = info["replicates"]
    assert 0 < S < 1024
    idx = np.sort(np.random.default_rng(20160415).choice(1024, S, replace=False))
    assert got["f_smooth"].shape == (S, 500, 8) and got["P_smooth"].shape == (S, 500, 36) and got["loglik"].shape == (S,)

    from dynamic_factor_models_amd import DfmContext
    ctx = DfmContext()
    try:
        panel, par = ctx.synth_panels(20160415, 0, 1024, 500, 200, 8)
        f, P, ll = ctx.ks_pass_batch(panel, *par, may_have_missing=False)
        ctx.synchronize()
        ix = torch.from_numpy(idx).to(panel.device)
        for name, t in (("f_smooth", f), ("P_smooth", P), ("loglik", ll)):
            assert np.array_equal(got[name], t.index_select(0, ix).cpu().numpy()), name
    finally:
        ctx.close()
