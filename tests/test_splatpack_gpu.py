"""`lara_amd.splatpack` on the device: every kernel's output equals its host twin's on all cases of tests/splatpack_cases.py as
integers -- the alpha byte and the importance key under the boundary rule of the CPU tests, fp32 words that went through exp / log
within one spacing -- twice, on a side stream, with outputs carved out of sentinel-filled buffers at odd row offsets; a packed and
unpacked 1 024-surfel scene renders, per output map, no more than 0.1 dB below the float64-restated round trip; tools/render_surfels.py
takes a compressed PLY and a ``.splat`` file.  Figures measured at writing: profiles/splatpack_parity.txt."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import splatpack_cases as C
from tests import splatpack_restate as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)


def _cloud(c, device=DEV):
    from lara_amd import splatio
    return splatio.SurfelCloud(*(torch.from_numpy(c[k].copy()).to(device) for k in C.FIELDS))


def _np(t):
    return t.detach().cpu().numpy()


def _carve(rows, tail, dtype, row0):
    """A sentinel-filled device buffer of row0 + rows + 2 rows and the ``rows`` rows at ``row0`` of it."""
    nbytes = torch.empty(0, dtype=dtype).element_size()
    width = int(np.prod(tail)) if tail else 1
    raw = torch.full(((row0 + rows + 2) * width * nbytes,), C.SENTINEL, dtype=torch.uint8, device=DEV)
    whole = raw.view(dtype).view((row0 + rows + 2,) + tuple(tail))
    return raw, whole[row0:row0 + rows], (row0 * width * nbytes, (row0 + rows) * width * nbytes)


def _intact(raw, span):
    b = _np(raw)
    return (b[:span[0]] == C.SENTINEL).all() and (b[span[1]:] == C.SENTINEL).all()


def _device_outputs(cloud, k, degree, row0):
    """Every kernel once: a dict of numpy outputs.  ``row0`` None: fresh tensors; else outputs carved out of sentinel buffers."""
    from lara_amd import splatpack as sp
    P, P_out, W, n = cloud.n_surfels, k["order"].shape[0], sp.sh_width(degree), (degree + 1) ** 2
    Cn = (P_out + 255) // 256
    guards = []

    def out(rows, tail, dtype):
        if row0 is None:
            return None
        raw, view, span = _carve(rows, tail, dtype, row0)
        guards.append((raw, span))
        return view
    valid, box, dropped = sp.bounds(cloud, out=out(P, (), torch.uint8))
    mk = sp.morton_keys(cloud, valid, box, out=out(P, (), torch.int64))
    ik = sp.importance_keys(cloud, valid, C.THICKNESS, out=out(P, (), torch.int64))
    order, sorder = torch.from_numpy(k["order"]).to(DEV), torch.from_numpy(k["splat_order"]).to(DEV)
    triple = None if row0 is None else (out(Cn, (18,), torch.float32), out(P_out, (4,), torch.int32), out(P_out, (W,), torch.uint8))
    chunks, words, sh = sp.encode(cloud, order, C.THICKNESS, out=triple)
    five = lambda deg: None if row0 is None else [out(P_out, t, torch.float32) for t in ((3,), ((deg + 1) ** 2, 3), (1,), (2,), (4,))]
    dec = sp.decode(chunks, words, sh, degree, out=five(degree))
    rows = sp.splat_encode(cloud, sorder, C.THICKNESS, out=out(P_out, (32,), torch.uint8))
    sdec = sp.splat_decode(rows, out=five(0))
    torch.cuda.current_stream(DEV).synchronize()
    res = dict(valid=_np(valid), box=_np(box), dropped=int(dropped), morton_keys=_np(mk), importance_keys=_np(ik), chunks=_np(chunks),
               words=_np(words).view(np.uint32), sh=_np(sh), decoded=[_np(t) for t in dec], splat=_np(rows).view(np.uint32).reshape(-1, 8),
               splat_decoded=[_np(t) for t in sdec])
    assert all(_intact(raw, span) for raw, span in guards), "a sentinel beside an output was overwritten"
    return res


def _host_outputs(c, k, degree):
    from lara_amd import splatpack as sp
    cloud = _cloud(c, "cpu")
    valid, box, dropped = sp.bounds(cloud)
    mk, ik = sp.morton_keys(cloud, valid, box), sp.importance_keys(cloud, valid, C.THICKNESS)
    chunks, words, sh = sp.encode(cloud, torch.from_numpy(k["order"]), C.THICKNESS)
    rows = sp.splat_encode(cloud, torch.from_numpy(k["splat_order"]), C.THICKNESS)
    return dict(valid=_np(valid), box=_np(box), dropped=int(dropped), morton_keys=_np(mk), importance_keys=_np(ik), chunks=_np(chunks),
                words=_np(words).view(np.uint32), sh=_np(sh), decoded=[_np(t) for t in sp.decode(chunks, words, sh, degree)],
                splat=_np(rows).view(np.uint32).reshape(-1, 8), splat_decoded=[_np(t) for t in sp.splat_decode(rows)])


def _compare(got, want, k, tally):
    """Device outputs against the host twin's."""
    for name in ("valid", "morton_keys", "sh"):
        assert np.array_equal(got[name], want[name]), name
    assert got["dropped"] == want["dropped"]
    for name in ("box", "chunks"):
        assert np.array_equal(got[name].view(np.uint32), want[name].view(np.uint32)), name
    tally["keys"] += C.exempt_keys(got["importance_keys"], want["importance_keys"], k["importance_pre"], k["valid"])
    pre, spre = k["alpha_pre"][k["order"]], k["alpha_pre"][k["splat_order"]]
    assert np.array_equal(got["words"][:, :3], want["words"][:, :3]) and np.array_equal(got["words"][:, 3] >> 8, want["words"][:, 3] >> 8)
    tally["alpha"] += C.exempt_bytes(got["words"][:, 3] & 255, want["words"][:, 3] & 255, pre)
    g, w = got["splat"], want["splat"]
    assert np.array_equal(g[:, [0, 1, 2, 5, 7]], w[:, [0, 1, 2, 5, 7]]) and np.array_equal(g[:, 6] & 0xFFFFFF, w[:, 6] & 0xFFFFFF)
    tally["alpha"] += C.exempt_bytes(g[:, 6] >> 24, w[:, 6] >> 24, spre)
    far, off = C.spacing_off(g[:, 3:5].copy().view(np.float32), w[:, 3:5].copy().view(np.float32))
    assert far == 0
    tally["exp_words"] += off
    # the decoders read what the DEVICE encoded: decode the host's words on the host only where they are the same words
    if np.array_equal(got["words"], want["words"]):
        for i, name in enumerate(C.FIELDS):
            if name in ("opacity",):                                   # (through log)
                far, off = C.spacing_off(got["decoded"][i], want["decoded"][i])
                assert far == 0
                tally["log_words"] += off
            else:
                assert np.array_equal(got["decoded"][i].view(np.uint32), want["decoded"][i].view(np.uint32)), name
    if np.array_equal(g, w):
        for i, name in enumerate(C.FIELDS):
            if name in ("opacity", "scales"):
                far, off = C.spacing_off(got["splat_decoded"][i], want["splat_decoded"][i])
                assert far == 0
                tally["log_words"] += off
            else:
                assert np.array_equal(got["splat_decoded"][i].view(np.uint32), want["splat_decoded"][i].view(np.uint32)), name


@pytest.mark.parametrize("degree", C.DEGREES)
def test_every_kernel_equals_its_host_twin(hip_lib, degree):
    side = torch.cuda.Stream(DEV)
    tally = dict(keys=0, alpha=0, exp_words=0, log_words=0)
    cases = [c for c in C.cases() if c[1] == degree]
    for P, _, kind in cases:
        k = C.case(P, degree, kind)
        want = _host_outputs(k["cloud"], k, degree)
        cloud = _cloud(k["cloud"])
        with torch.cuda.stream(side):
            for attempt in range(2):
                _compare(_device_outputs(cloud, k, degree, None), want, k, tally)
                for row0 in C.ROW_OFFSETS:
                    _compare(_device_outputs(cloud, k, degree, row0), want, k, tally)
        side.synchronize()
    print(f"splatpack parity, kernels against the host entries, SH degree {degree}, {len(cases)} cases, twice, on a side stream, fresh and "
          f"carved outputs: alpha bytes that differ {tally['alpha']}, importance keys that differ {tally['keys']}, .splat exp words that "
          f"differ {tally['exp_words']}, decoded log words that differ {tally['log_words']} (all within the rules); everything else equal, "
          f"every sentinel intact")


def test_pack_and_unpack_on_the_device(hip_lib):
    """The public route on the device against the same route on the host: the Morton order comes from the device's own sort."""
    from lara_amd import splatpack as sp
    for P, degree, kind in ((1000, 3, "mixed"), (257, 1, "coincident"), (300, 1, "all_invalid"), (0, 1, "mixed")):
        k = C.case(P, degree, kind)
        dev, host = sp.pack(_cloud(k["cloud"]), C.THICKNESS), sp.pack(_cloud(k["cloud"], "cpu"), C.THICKNESS)
        assert dev.device.type == "cuda" and dev.dropped == host.dropped == k["dropped"] and dev.n_surfels == P - k["dropped"]
        assert np.array_equal(_np(dev.order), k["order"]) and np.array_equal(_np(host.order), k["order"])
        assert np.array_equal(_np(dev.chunks).view(np.uint32), k["chunks"].view(np.uint32)) and np.array_equal(_np(dev.sh), k["sh"])
        assert np.array_equal(_np(dev.words).view(np.uint32)[:, :3], k["words"][:, :3])
        cloud, info = sp.unpack(dev)
        assert cloud.n_surfels == dev.n_surfels and cloud.sh_degree == degree and cloud.device.type == "cuda"
        assert all(bool(torch.isfinite(t).all()) for t in cloud.render_args())
        rows, order, gone = sp.splat_rows(_cloud(k["cloud"]), C.THICKNESS)
        assert gone == k["dropped"] and rows.shape == (P - gone, 32) and rows.device.type == "cuda"


# ------------------------------------------------------------------------------------------------------------------ renders

def test_a_round_trip_renders_as_the_restated_round_trip(hip_lib):
    from lara_amd import splatio, splatpack as sp
    from tests import test_splatxform_gpu as X
    s = X._scene()
    original, cloud = s["original"], s["cloud"]
    c = {k: _np(t) for k, t in zip(C.FIELDS, cloud.render_args())}
    pl = S.plan(C.THICKNESS)
    valid, box, dropped = S.bounds(c)
    assert dropped == 0
    order = S.order_of(S.morton_keys(c, valid, box), dropped)
    restated = S.decode(*S.encode(c, order, pl), 3)
    restated = splatio.SurfelCloud(*(torch.from_numpy(np.ascontiguousarray(S.f32(restated[k]))).to(DEV) for k in C.FIELDS))
    routes = {"restated": restated, "device": sp.unpack(sp.pack(cloud, C.THICKNESS))[0],
              "host": sp.unpack(sp.pack(cloud.to("cpu"), C.THICKNESS))[0].to(DEV)}
    psnr = {name: {m: X._psnr(r[m], original[m]) for m in X.MAPS} for name, r in
            ((name, X._render(cl, s["cams"], s["c2w"])) for name, cl in routes.items())}
    for m in X.MAPS:
        print(f"splatpack parity, 1 024 surfels of SH degree 3, two 64 x 64 views, pack then unpack against the original render, {m}: "
              f"restated {psnr['restated'][m]:.2f} dB, device {psnr['device'][m]:.2f} dB, host {psnr['host'][m]:.2f} dB")
    for m in X.MAPS:
        assert psnr["device"][m] >= psnr["restated"][m] - 0.1, (m, psnr["device"][m], psnr["restated"][m])
        assert psnr["host"][m] >= psnr["restated"][m] - 0.1, (m, psnr["host"][m], psnr["restated"][m])


def test_render_surfels_tool_takes_the_packed_files(hip_lib, tmp_path):
    from lara_amd import splatpack as sp
    from tests import test_splatxform_gpu as X
    s = X._scene()
    for name in ("scene.compressed.ply", "scene.splat"):
        path, out = str(tmp_path / name), tmp_path / name.split(".")[1]
        assert sp.write(path, s["cloud"]) == os.path.getsize(path)
        # a fresh child process under its own time limit; nothing below runs when it fails
        run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "render_surfels.py"), path,
                              "--dataset", "gobjeverse", "--out", str(out), "--quick"], capture_output=True, text=True, cwd=ROOT)
        assert run.returncode == 0, run.stderr[-2000:]
        names = sorted(n for n in os.listdir(out) if n.endswith(".png"))
        assert names == ["normal_0000.png", "normal_0001.png", "rgb_0000.png", "rgb_0001.png"]
        assert f'"n_surfels": {s["cloud"].n_surfels}' in run.stdout
