"""Generates tests/golden/loader_raw_ref.npz: items of the REFERENCE's own dataset class (dataLoader/gobjverse.py:17-146) taken
over by `lara_amd.dataset.raw_views`, on the in-memory scene store, with the seeds and the three configurations of
tests/golden/make_loader_fixture.py (train / 4 groups, test / 4 groups, test / 1 group; the first and the last index, 32 x 32), so
that tests/test_batchfinish.py can hold them against the class's own items (loader_ref.npz) field by field.  The ray maps are left
out: they are the class's own and loader_ref.npz has them.  Run where a LaRa checkout is available:
    python tests/golden/make_loader_raw_fixture.py <path of the LaRa checkout>
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

out = {}
for split, n_group, tag in (("train", 4, "train4"), ("test", 4, "test4"), ("test", 1, "test1")):
    cfg = types.SimpleNamespace(data_root="mem", split=split, img_size=(32, 32), n_group=n_group, n_scenes=100, load_normal=True)
    before = dict(vars(cfg))
    ds = dataset.raw_views(ref.gobjverse(cfg))
    assert vars(cfg) == before
    out[f"{tag}.len"] = np.array(len(ds))
    for index in (0, len(ds) - 1):
        random.seed(100 + index)
        torch.manual_seed(200 + index)
        for k, v in ds[index].items():
            if k == "meta":
                out[f"{tag}.{index}.scene"] = np.array(str(v["scene"]))
                out[f"{tag}.{index}.tar_view"] = np.array(v["tar_view"])
            elif k not in dataset.RAY_KEYS:
                out[f"{tag}.{index}.{k}"] = np.asarray(v)
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "loader_raw_ref.npz"), **out)
print("wrote", len(out), "arrays")
