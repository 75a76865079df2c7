"""CPU tests of the point-cloud evaluation (mvsnet_amd/evaluate.py): the float64 reference on a hand-computed case and
against cKDTree, the preprocessing statements, the general PLY vertex reader, the argument checks of the mvs_nn / stats /
voxel entry points (no GPU call) and the command line without a GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import pointcloud_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hand_computed_metrics():
    from mvsnet_amd import evaluate as E
    pred = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 3], [10, 0, 0]], np.float32)
    gt = np.array([[0, 0, 0.5], [1, 0, 0], [0, 2, 0]], np.float32)
    md = 2.0
    dp, ip, _, _ = R.nearest(pred, gt, md)
    # (0,0,0) -> (0,0,.5) 0.5; (1,0,0) -> itself 0; (0,0,3) -> (0,0,.5) 2.5 beyond; (10,0,0) beyond
    assert np.allclose(dp, [0.5, 0.0, np.inf, np.inf]) and ip.tolist() == [0, 1, -1, -1]
    dg, ig, _, _ = R.nearest(gt, pred, md)
    # (0,0,.5) -> (0,0,0) 0.5; (1,0,0) -> 0; (0,2,0) -> (0,0,0) exactly 2.0 = max_dist: found, but an outlier
    assert np.allclose(dg, [0.5, 0.0, 2.0]) and ig.tolist() == [0, 1, 0]
    m = R.metrics(dp, dg, md, (0.25, 1.0))
    assert m["accuracy"] == 0.25 and m["accuracy_inlier_fraction"] == 0.5 and m["accuracy_median"] == 0.25
    assert m["completeness"] == 0.25 and m["completeness_inlier_fraction"] == 2 / 3
    assert m["overall"] == 0.25
    assert m["precision"] == [0.25, 0.5] and m["recall"] == [1 / 3, 2 / 3]
    assert m["fscore"][0] == pytest.approx(2 * 0.25 * (1 / 3) / (0.25 + 1 / 3))
    assert m["fscore"][1] == pytest.approx(2 * 0.5 * (2 / 3) / (0.5 + 2 / 3))
    # the library's assembly of the same counts
    e = E.metrics_from_counts(4, 3, (0.5, 2, [1, 2]), (0.5, 2, [1, 2]), (0.25, 1.0), 0.25, 0.25)
    for k in ("accuracy", "accuracy_inlier_fraction", "completeness", "completeness_inlier_fraction", "overall", "precision",
              "recall"):
        assert e[k] == m[k], k
    assert e["fscore"] == pytest.approx(m["fscore"])
    assert E.metrics_from_counts(2, 2, (0.0, 0, [0]), (0.0, 0, [0]), (1.0,))["fscore"] == [0.0]
    assert E.inlier_median(np.array([3.0, np.inf, 1.0, 2.0, 5.0], np.float32), 4.0) == 2.0


def test_reference_matches_ckdtree():
    spatial = pytest.importorskip("scipy.spatial")
    q = R.noisy(R.plane_sphere(3000, seed=1), 0.5, seed=2)
    t = R.plane_sphere(4000, seed=3)
    d, idx, d_all, gap = R.nearest(q, t, 2.0)
    dd, ii = spatial.cKDTree(t.astype(np.float64)).query(q.astype(np.float64), k=2)
    assert np.allclose(d_all, dd[:, 0], rtol=0, atol=1e-12)
    assert np.array_equal(idx[np.isfinite(d)], ii[np.isfinite(d), 0])
    assert np.array_equal(np.isfinite(d), dd[:, 0] <= 2.0)
    assert np.allclose(gap, dd[:, 1] - dd[:, 0], atol=1e-12)


def test_voxel_first_in_order_crop_and_transform_rules():
    from mvsnet_amd import evaluate as E
    p = R.uniform(5000, 0.0, 10.0, seed=4)
    keep = R.voxel_first(p, 1.3)
    # independent statement: walk the input, keep a point when its voxel is new
    seen, want = set(), []
    m = p.astype(np.float64).min(0)
    for x in p:
        k = tuple(np.floor((x.astype(np.float64) - m) / 1.3).astype(int))
        if k not in seen:
            seen.add(k)
            want.append(x)
    assert np.array_equal(keep, np.array(want))
    # crop is inclusive on both faces, compared in float64
    box = np.array([[1, 1, 1], [2, 2, 2], [2.5, 1, 1], [1, 1, 0.9999999]], np.float32)
    assert np.array_equal(R.crop(box, (1, 1, 1), (2, 2, 2)), box[:2])
    assert E.check_crop((1, 1, 1, 2, 2, 2))[0].tolist() == [1, 1, 1]
    with pytest.raises(ValueError):
        E.check_crop((1, 1, 1, 0, 2, 2))
    T = np.eye(4)
    T[:3, 3] = [1, 2, 3]
    assert np.array_equal(R.transform(box, T), (box.astype(np.float64) + [1, 2, 3]).astype(np.float32))
    T[3, 0] = 1e-9
    for bad in (T, np.eye(3)):
        with pytest.raises(ValueError):
            E.check_transform(bad)
    # refused before any device work, with or without a GPU
    with pytest.raises(ValueError, match="affine"):
        E.evaluate_point_clouds(p, p, max_dist=1.0, transform=T)
    with pytest.raises(ValueError, match="threshold"):
        E.evaluate_point_clouds(p, p, max_dist=1.0, thresholds=(0.5, 1.5))
    with pytest.raises(ValueError):
        E.check_thresholds((0.0,), 1.0)
    with pytest.raises(ValueError):
        E.check_thresholds((), float("inf"))


def _ply_bytes(fmt, props, rows, faces=None, vertex_first=True):
    """A PLY file built by hand: props [(type, name)], rows of values; optional triangle faces."""
    head = ["ply", "format %s 1.0" % fmt, "comment built in a test"]
    vert = ["element vertex %d" % len(rows)] + ["property %s %s" % p for p in props]
    face = ["element face %d" % len(faces), "property list uchar int vertex_indices"] if faces is not None else []
    head += (vert + face) if vertex_first else (face + vert)
    head.append("end_header")
    out = ("\n".join(head) + "\n").encode("ascii")
    np_types = {"float": "f4", "double": "f8", "uchar": "u1", "uint8": "u1", "int16": "i2", "int": "i4", "float32": "f4"}
    end = {"binary_little_endian": "<", "binary_big_endian": ">"}.get(fmt)

    def vertices():
        if end is None:
            return "".join(" ".join(repr(v) for v in r) + "\n" for r in rows).encode()
        dt = np.dtype([(n, end + np_types[t]) for t, n in props])
        return np.array([tuple(r) for r in rows], dt).tobytes()

    def face_bytes():
        if faces is None:
            return b""
        if end is None:
            return "".join("3 %d %d %d\n" % tuple(f) for f in faces).encode()
        return b"".join(np.array([3], "u1").tobytes() + np.array(f, end + "i4").tobytes() for f in faces)
    return out + (vertices() + face_bytes() if vertex_first else face_bytes() + vertices())


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
def test_read_ply_points_formats_extra_properties_and_faces(tmp_path, fmt):
    from mvsnet_amd import evaluate as E
    props = [("float", "x"), ("float", "y"), ("double", "z"), ("float32", "nx"), ("float", "ny"), ("float", "nz"),
             ("uchar", "red"), ("uint8", "green"), ("uchar", "blue"), ("uchar", "alpha"), ("int16", "label")]
    rows = [[0.5, -1.25, 3.0, 0, 0, 1, 10, 20, 30, 255, -4], [2.0, 0.125, -7.5, 1, 0, 0, 40, 50, 60, 128, 9],
            [1e-3, 4.0, 0.0, 0, 1, 0, 70, 80, 90, 0, 0]]
    for vertex_first in (True, False):
        path = str(tmp_path / ("a%d.ply" % vertex_first))
        open(path, "wb").write(_ply_bytes(fmt, props, rows, faces=[[0, 1, 2], [2, 1, 0]], vertex_first=vertex_first))
        xyz, rgb = E.read_ply_points(path)
        assert xyz.dtype == np.float32 and rgb.dtype == np.uint8
        assert np.array_equal(xyz, np.array([r[:3] for r in rows], np.float32))
        assert rgb.tolist() == [r[6:9] for r in rows]
    path = str(tmp_path / "plain.ply")
    open(path, "wb").write(_ply_bytes(fmt, [("double", "x"), ("double", "y"), ("double", "z")], [[1.0, 2.0, 3.0]]))
    xyz, rgb = E.read_ply_points(path)
    assert xyz.tolist() == [[1.0, 2.0, 3.0]] and rgb is None


def test_read_ply_points_reads_write_ply_and_rejects_bad_vertices(tmp_path):
    from mvsnet_amd import evaluate as E, fusion as F
    rs = np.random.RandomState(0)
    xyz = rs.standard_normal((50, 3)).astype(np.float32)
    rgb = rs.randint(0, 256, (50, 3)).astype(np.uint8)
    F.write_ply(str(tmp_path / "w.ply"), xyz, rgb)
    x2, c2 = E.read_ply_points(str(tmp_path / "w.ply"))
    assert np.array_equal(x2, xyz) and np.array_equal(c2, rgb)
    bad = _ply_bytes("ascii", [("float", "x"), ("float", "y")], [[1.0, 2.0]])
    open(str(tmp_path / "noz.ply"), "wb").write(bad)
    with pytest.raises(ValueError, match="without z"):
        E.read_ply_points(str(tmp_path / "noz.ply"))
    listed = (b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
              b"property list uchar int extra\nend_header\n1 2 3 2 5 6\n")
    open(str(tmp_path / "list.ply"), "wb").write(listed)
    with pytest.raises(ValueError, match="list property"):
        E.read_ply_points(str(tmp_path / "list.ply"))


def test_entry_points_check_arguments_without_gpu(lib_built):
    import ctypes
    from mvsnet_amd import _lib
    h = _lib.load()
    BADARG, SHAPE, WORKSPACE = -1, -2, -3
    assert h.mvs_nn_workspace_bytes(100, 200, 4, 4, 4) > 0
    assert h.mvs_nn_workspace_bytes(100, 200, 0, 4, 4) == 0
    assert h.mvs_nn_workspace_bytes(-1, 200, 4, 4, 4) == 0
    assert h.mvs_nn_workspace_bytes(100, 200, 1 << 10, 1 << 10, 1 << 10) == 0
    nz = 4096                                  # never dereferenced: the checks return before any HIP call
    ws = h.mvs_nn_workspace_bytes(100, 200, 4, 4, 4)

    def nn(**kw):
        a = dict(q=nz, nq=100, t=nz, nt=200, cell=1.0, gx=4, gy=4, gz=4, md=2.0, dist=nz, idx=nz, ws=nz, wsb=ws)
        a.update(kw)
        return h.mvs_nn_f32(a["q"], a["nq"], a["t"], a["nt"], 0.0, 0.0, 0.0, a["cell"], a["gx"], a["gy"], a["gz"], a["md"],
                            a["dist"], a["idx"], a["ws"], a["wsb"], None)
    assert nn(q=None) == BADARG and nn(t=None) == BADARG and nn(dist=None) == BADARG and nn(ws=None) == BADARG
    assert nn(nq=-5) == BADARG and nn(nt=0) == BADARG
    assert nn(gx=0) == BADARG and nn(cell=0.0) == BADARG and nn(md=-1.0) == BADARG and nn(md=float("inf")) == BADARG
    assert nn(gx=1 << 10, gy=1 << 10, gz=1 << 10) == SHAPE
    assert nn(wsb=ws - 1) == WORKSPACE
    thr = (ctypes.c_float * 3)(0.5, 1.0, 2.0)
    assert h.mvs_dist_stats_workspace_bytes(1000, 3) > 0 and h.mvs_dist_stats_workspace_bytes(1000, 17) == 0
    sws = h.mvs_dist_stats_workspace_bytes(1000, 3)
    st = lambda **kw: h.mvs_dist_stats_f32(kw.get("d", nz), kw.get("n", 1000), kw.get("md", 2.0), kw.get("thr", thr),
                                           kw.get("nt", 3), kw.get("out", nz), nz, kw.get("wsb", sws), None)
    assert st(d=None) == BADARG and st(out=None) == BADARG and st(n=-1) == BADARG and st(thr=None) == BADARG
    assert st(md=1.5) == BADARG                                   # tau = 2 > max_dist
    assert st(thr=(ctypes.c_float * 3)(0.0, 1.0, 2.0)) == BADARG
    assert st(thr=(ctypes.c_float * 17)(*([1.0] * 17)), nt=17) == SHAPE
    assert st(wsb=sws - 1) == WORKSPACE
    assert h.mvs_voxel_keys_f32(None, 10, 0.0, 0.0, 0.0, 1.0, nz, None) == BADARG
    assert h.mvs_voxel_keys_f32(nz, 10, 0.0, 0.0, 0.0, 0.0, nz, None) == BADARG
    vws = h.mvs_voxel_select_workspace_bytes(10)
    assert vws > 0 and h.mvs_voxel_select_workspace_bytes(0) == 0
    assert h.mvs_voxel_select_f32(nz, 10, nz, None, nz, nz, nz, vws, None) == BADARG
    assert h.mvs_voxel_select_f32(nz, 10, nz, nz, nz, nz, nz, vws - 1, None) == WORKSPACE


def test_cli_without_gpu_fails_clearly(tmp_path):
    from mvsnet_amd import fusion as F
    F.write_ply(str(tmp_path / "a.ply"), np.zeros((3, 3), np.float32), np.zeros((3, 3), np.uint8))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-m", "mvsnet_amd.evaluate", "--pred", str(tmp_path / "a.ply"), "--gt",
                        str(tmp_path / "a.ply"), "--max_dist", "1", "--out", str(tmp_path / "m.json")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "needs a GPU" in r.stderr and "Traceback" not in r.stderr
    assert not os.path.exists(str(tmp_path / "m.json"))
