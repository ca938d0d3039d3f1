"""Generates tests/golden/loader_hooked_ref.npz: items of the REFERENCE's own dataset class (dataLoader/gobjverse.py:17-146)
with `lara_amd.dataset.skip_cpu_rays` applied to its module, on the in-memory scene store and with the seeds of
tests/golden/make_loader_fixture.py (split "test", 4 groups, the first and the last index), so that tests/test_loader.py
can hold them against the class's items without the hook (loader_ref.npz).  Run where a LaRa checkout is available:
    python tests/golden/make_loader_hook_fixture.py <path of the LaRa checkout>
"""
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.path.abspath(sys.argv[1])
sys.path.insert(0, ROOT)
from lara_amd import dataset  # noqa: E402
from tests.helpers_store import make_store  # noqa: E402

store = make_store(seed=5)
h5 = types.ModuleType("h5py")
h5.File = lambda path, mode="r": store
sys.modules["h5py"] = h5
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
# a bare package: only the loader module itself (and dataLoader.utils) is executed, as in make_loader_fixture.py
pkg = types.ModuleType("dataLoader")
pkg.__path__ = [os.path.join(REF, "dataLoader")]
sys.modules["dataLoader"] = pkg
sys.path.insert(0, REF)
import dataLoader.gobjverse as ref  # noqa: E402

dataset.skip_cpu_rays(ref)
cfg = types.SimpleNamespace(data_root="mem", split="test", img_size=(32, 32), n_group=4, n_scenes=100, load_normal=True)
ds = ref.gobjverse(cfg)
out = {"test4.len": np.array(len(ds))}
for index in (0, len(ds) - 1):
    random.seed(100 + index)
    torch.manual_seed(200 + index)
    for k, v in ds[index].items():
        if k == "meta":
            out[f"test4.{index}.scene"] = np.array(str(v["scene"]))
            out[f"test4.{index}.tar_view"] = np.array(v["tar_view"])
        else:
            out[f"test4.{index}.{k}"] = np.asarray(v)
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "loader_hooked_ref.npz"), **out)
print("wrote", len(out), "arrays")
