"""A tuning build runs beside the installed library, not over it (MI355X; skipped without hipcc): the -DTC_STAMPS variant of
tail_chain against the default build in two fresh processes, one after the other, on what smoke() runs first -- the tiny
config, fixed seeds, 512 pairs, D = 64, score_pairs(logits=True) + check_selection(); the step ends in
lpf_tail_chain_merge_f32, so the stamped kernel is on the path.  The stamps add clock reads and stores and no arithmetic:
the logits are the same bit for bit, and the installed library's bytes do not change."""
import json
import subprocess
import sys

import numpy as np
import pytest

from lpformer_amd import _lib
from tests.test_variant_build_host import ROOT, build_stamped_variant, clean_env, sha256, tail_isa

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(tail_isa.find_hipcc() is None, reason="needs hipcc")]

# LPF_HIP_LIB set: a zeroed stamp buffer (sized as in tools/tail_stamps.py: workgroups x wavefronts x 16 words -- this
# batch launches 8 workgroups) goes to the variant's setter before scoring.
CHILD = """
import ctypes, json, os
import numpy as np, torch
import lpformer_amd
from lpformer_amd import data as D, _lib
cfg = D.CONFIGS["tiny"]
n, dev = cfg["n"], torch.device("cuda:0")
ei, w = D.chung_lu_graph(n, cfg["edges"], seed=1, max_weight=cfg["max_weight"])
x = np.random.default_rng(0).standard_normal((n, cfg["f_in"])).astype(np.float32)
data = D.build_data(ei, x, n, edge_weight=w, eps=cfg["eps"])
torch.manual_seed(0)
model = lpformer_amd.LinkTransformer(D.train_args_for(cfg), data, device=dev).to(dev).eval()
score = lpformer_amd.mlp_score(model.out_dim, model.out_dim, 1, 2).to(dev).eval()
batch = torch.from_numpy(D.sample_pairs(ei, n, 512, seed=3)).to(dev)
assert model.dim == 64
stamps = None
if os.environ.get("LPF_HIP_LIB"):
    fn = _lib.hip().lpf_tail_chain_set_stamps
    fn.argtypes, fn.restype = [ctypes.c_void_p], ctypes.c_int
    stamps = torch.zeros(2048 * 8 * 16, dtype=torch.int64, device=dev)
    assert fn(stamps.data_ptr()) == 0
lg = model.score_pairs(batch, model.propagate(), score, logits=True)
assert model.check_selection()
torch.cuda.synchronize()
print(json.dumps({"lib": _lib.HIP_LIB_PATH, "stamps": None if stamps is None else int((stamps != 0).sum()),
                  "logits": lg.cpu().numpy().view(np.uint32).tolist()}))
"""


def _child(lib):
    env = clean_env() if lib is None else clean_env(LPF_HIP_LIB=lib)
    p = subprocess.run([sys.executable, "-c", CHILD], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])     # (the next child starts only after this one passed)
    return json.loads(p.stdout.splitlines()[-1])


def test_stamped_variant_runs_beside_the_installed_library():
    before, variant = build_stamped_variant()
    a = _child(None)
    b = _child(variant)
    print("installed:", a["lib"], " variant:", b["lib"], " non-zero stamp words:", b["stamps"])
    assert a["lib"] == _lib.INSTALLED_HIP_LIB_PATH and a["stamps"] is None
    assert b["lib"] == variant != a["lib"]
    assert b["stamps"] > 0
    assert sha256(_lib.INSTALLED_HIP_LIB_PATH) == before
    la, lb = (np.array(r["logits"], dtype=np.uint32).view(np.float32) for r in (a, b))
    assert la.shape == (512,) and np.isfinite(la).all()
    print("max |logit difference|:", float(np.abs(la - lb).max()))
    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32))
