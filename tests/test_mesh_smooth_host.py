"""No GPU: tests/mesh_smooth_reference.py, the numpy restatement of mvsnet_amd/mesh_smooth.py, held to facts that were worked
out by hand or follow from the semantics (a hexagon fan under the three boundary modes, shrinkage of a noisy sphere under
Laplacian relaxation and its absence under Taubin's pair, the bound on the displacement, edge multiplicities and the counts of
the report), the option checks of the module and of the three command lines, and the argument checks of the entry points,
which come before any GPU call."""
import ctypes

import numpy as np
import pytest

from tests import mesh_smooth_reference as R


def _d(x):
    return np.asarray(x, np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the hexagon fan, by hand

def test_hexagon_fan_free_moves_the_hub_by_lambda_times_the_rim_mean():
    v, f = R.fan(6)
    lam = 0.25
    out = R.smooth(v, None, f, 1, lam, 0.0, "free")[0]
    s = np.zeros(3)
    for j in range(1, 7):                                                      # ascending, one after the other
        s = s + _d(v[j])
    want = (_d(v[0]) + np.float64(np.float32(lam)) * (s / 6.0 - _d(v[0]))).astype(np.float32)
    assert out[0].tobytes() == want.tobytes()
    assert np.abs(out[0] - (v[0] + lam * (v[1:].mean(0) - v[0]))).max() < 1e-6
    # a rim vertex has three neighbours: the hub and its two rim neighbours
    want1 = (_d(v[1]) + 0.25 * (((_d(v[0]) + _d(v[2])) + _d(v[6])) / 3.0 - _d(v[1]))).astype(np.float32)
    assert out[1].tobytes() == want1.tobytes()


def test_hexagon_fan_fixed_keeps_the_rim_and_moves_the_hub():
    v, f = R.fan(6)
    out, _, _, rep = R.smooth(v, None, f, 3, boundary="fixed")
    assert out[1:].tobytes() == v[1:].tobytes() and not np.array_equal(out[0], v[0])
    assert (rep["boundary_vertices"], rep["fixed_vertices"], rep["boundary_edges"], rep["edges"]) == (6, 6, 6, 12)
    free = R.smooth(v, None, f, 1, 0.5, 0.0, "free")[0]
    fixed = R.smooth(v, None, f, 1, 0.5, 0.0, "fixed")[0]
    assert free[0].tobytes() == fixed[0].tobytes()                             # the hub's pass is the same; Jacobi: it sees the old rim


def test_hexagon_fan_curve_averages_the_two_rim_neighbours_only():
    v, f = R.fan(6)
    adj = R.adjacency(v, f, "curve")
    assert adj["vertex_class"].tolist() == [R.INTERIOR] + [R.CURVE] * 6
    out = R.smooth(v, None, f, 1, 0.5, 0.0, "curve")[0]
    for j in range(1, 7):
        a, b = sorted((1 + (j - 2) % 6, 1 + j % 6))
        want = (_d(v[j]) + 0.5 * ((_d(v[a]) + _d(v[b])) / 2.0 - _d(v[j]))).astype(np.float32)
        assert out[j].tobytes() == want.tobytes(), j
    assert (out[1:, 2] == 0).all()                                             # the rim stays in its plane: the hub does not pull


# ------------------------------------------------------------------------------------------------ the noisy sphere

def test_laplacian_shrinks_the_noisy_sphere_and_taubin_does_not():
    v, f = R.sphere(16, 24)
    assert (len(v), len(f)) == (362, 720)
    noisy = (v * (1 + 0.02 * np.random.RandomState(3).randn(len(v)))[:, None]).astype(np.float32)
    radius = lambda x: np.linalg.norm(x.astype(np.float64), axis=1)
    r_in = radius(noisy)
    lap, _, _, rep = R.smooth(noisy, None, f, 10, 0.5, 0.0)
    tau = R.smooth(noisy, None, f, 10, 0.5, -0.53)[0]
    print("input: mean %.4f std %.4f; laplacian: mean %.4f; taubin: mean %.4f std %.4f"
          % (r_in.mean(), r_in.std(), radius(lap).mean(), radius(tau).mean(), radius(tau).std()))
    assert rep["boundary_edges"] == 0 and rep["fixed_vertices"] == 0 and rep["edges"] == 1080 and rep["non_manifold_edges"] == 0
    assert radius(lap).mean() < 0.95
    assert abs(radius(tau).mean() - 1) < 0.02 and radius(tau).std() < 0.5 * r_in.std()


# ------------------------------------------------------------------------------------------------ the bound, dead vertices and faces

def test_the_bound_holds_and_dead_vertices_keep_their_bytes():
    v, f = (x.copy() for x in R.grid(12))
    v[:, 2] += (0.2 * np.random.RandomState(1).randn(len(v))).astype(np.float32)
    lone = np.array([[5, 5, 5], [np.nan, 1, 2]], np.float32)                   # an isolated vertex and one that no face names
    v = np.concatenate([v, lone])
    v[20, 1], v[77, 0], v[100, 2] = np.nan, np.inf, -np.inf
    n = len(v)
    f = np.concatenate([f, np.array([[-1, 0, 1], [0, 1, n], [3, 2 ** 31 - 1, 4]], np.int32)])
    r = np.float32(0.01)
    out, _, ff, rep = R.smooth(v, None, f, 4, boundary="free", max_displacement=r)
    free = R.smooth(v, None, f, 4, boundary="free")[0]
    dead = [20, 77, 100, n - 2, n - 1]
    assert out[dead].tobytes() == v[dead].tobytes() and free[dead].tobytes() == v[dead].tobytes()
    live = np.setdiff1d(np.arange(n), dead)
    moved = np.abs(free[live].astype(np.float64) - v[live])
    assert moved.max() > 10 * r                                                # without the bound the vertices go much farther
    bound = _d(r) + np.abs(_d(v[live])) * 2.0 ** -24 + 2.0 ** -149             # r plus one float32 rounding of the bound
    assert (np.abs(out[live].astype(np.float64) - _d(v[live])) <= bound).all()
    assert (np.abs(out[live].astype(np.float64) - _d(v[live])) >= 0.99 * r).any()
    assert (rep["invalid_faces"], rep["non_finite_vertices"]) == (3, 4) and ff.tobytes() == f.tobytes()
    without = R.adjacency(v, f[:-3], "free")
    assert np.array_equal(without["neighbours"], R.adjacency(v, f, "free")["neighbours"])          # invalid faces add no edge
    assert (R.edge_keys(v, f)[0][-18:] == R.DEAD).all()


def test_a_value_near_float_max_keeps_its_old_position():
    v, f = R.near_float_max()
    lam = 2.0 ** -20
    ys = R.passes(v, f, 1, lam, -1.0, "free")[1]
    assert len(ys) == 2 and np.isfinite(ys[0]).all() and (ys[0][:, 0] != v[:, 0]).all()            # the first pass moves every vertex
    # second pass, vertex 0 on x: its neighbours' mean is about -3e38, so y = x - (m - x) is about 9e38, beyond float32: the
    # vertex keeps the first pass's position on all three axes, also on y, where the result (1/2 + ...) was finite
    assert ys[1][0].tobytes() == ys[0][0].tobytes() and ys[0][0, 1] != 0
    assert ys[1].tobytes() == ys[0].tobytes()                                  # the other two overflow on x as well
    assert R.smooth(v, None, f, 1, lam, -1.0, "free")[0].tobytes() == ys[0].tobytes()


# ------------------------------------------------------------------------------------------------ multiplicities and the report

def test_edge_multiplicities():
    v, f = R.doubled_face()
    adj = R.adjacency(v, f)
    assert adj["multiplicity"].tolist() == [2] * 6 and adj["boundary_edges"] == 0 and adj["boundary_vertices"] == 0
    assert adj["non_manifold_edges"] == 0 and adj["edges"] == 3 and adj["vertex_class"].tolist() == [R.INTERIOR] * 3
    assert (adj["neighbours"] >= 0).all()
    v, f = R.three_on_one_edge()
    adj = R.adjacency(v, f)
    assert (adj["non_manifold_edges"], adj["boundary_edges"], adj["edges"], adj["boundary_vertices"]) == (1, 6, 7, 5)
    assert sorted(adj["multiplicity"].tolist()) == [1] * 12 + [3] * 2
    assert adj["neighbours"][:4].tolist() == [1, 2 - 2 ** 31, 3 - 2 ** 31, 4 - 2 ** 31]            # vertex 0: 1 (not boundary), 2, 3, 4
    assert adj["row_start"].tolist() == [0, 4, 8, 10, 12, 14]


def test_report_counts_on_the_grid_with_a_hole():
    n, gap = 6, 3
    v, f = R.grid(n, gap)                                                      # rows 2 and 5 of the quads are left out: two strips of 2 x 6
    _, _, _, rep = R.smooth(v, None, f, 1)
    quads = 2 * 2 * n
    # a strip of 2 x 6 quads: 3 x 6 horizontal + 2 x 7 vertical + 12 diagonal edges, 2 x 6 + 2 x 2 of them on its border
    assert rep["faces"] == 2 * quads and rep["edges"] == 2 * (18 + 14 + 12) and rep["boundary_edges"] == 2 * 16
    assert rep["boundary_vertices"] == 2 * 16 and rep["non_manifold_edges"] == 0 and rep["invalid_faces"] == 0
    assert rep["fixed_vertices"] == 2 * 16 + 7                                 # the last row of vertices has no face
    assert R.smooth(v, None, f, 1, boundary="free")[3]["fixed_vertices"] == 7
    assert set(rep) == set(__import__("mvsnet_amd.mesh_smooth", fromlist=["x"]).REPORT_FIELDS)


def test_intermediate_arrays_are_consistent():
    v, f = (x.copy() for x in R.grid(5))
    f[3] = [0, 1, 99]
    adj = R.adjacency(v, f, "curve")
    E, U = 6 * len(f), adj["U"]
    assert adj["keys"].shape == (E,) and adj["head"].sum() == U == adj["head_rank"][-1] == adj["row_start"][-1]
    assert (adj["keys"].reshape(-1, 6)[3] == R.DEAD).all()
    for vtx in range(len(v)):
        row = adj["neighbours"][adj["row_start"][vtx]:adj["row_start"][vtx + 1]] & (2 ** 31 - 1)
        assert (np.diff(row) > 0).all()
        live = adj["keys"][adj["keys"] != R.DEAD]
        assert set(row.tolist()) == set((live[(live >> 31) == vtx] & (2 ** 31 - 1)).tolist())


# ------------------------------------------------------------------------------------------------ options and command lines

def test_option_checks_come_before_any_gpu_work():
    from mvsnet_amd import mesh, mesh_smooth
    assert mesh_smooth.check_options(3) == (3, 0.5, float(np.float32(-0.53)), "fixed", None)
    assert mesh_smooth.check_options(1000, 1, -1, "curve", 0.1) == (1000, 1.0, -1.0, "curve", float(np.float32(0.1)))
    assert mesh_smooth.check_options(np.int64(2), np.float32(0.25), 0, "free", 2) == (2, 0.25, 0.0, "free", 2.0)
    v, f = np.ones((4, 3), np.float32), np.zeros((1, 3), np.int32)
    bad = [dict(iterations=0), dict(iterations=1001), dict(iterations=-1), dict(iterations=1.5), dict(iterations=True), dict(iterations="3"),
           dict(iterations=None), dict(lam=0), dict(lam=-0.5), dict(lam=1.5), dict(lam=np.nan), dict(lam=1e-60), dict(lam="x"),
           dict(lam=None), dict(lam=True), dict(mu=0.1), dict(mu=-1.5), dict(mu=np.nan), dict(mu=-np.inf), dict(mu="x"), dict(mu=None),
           dict(boundary="open"), dict(boundary=None), dict(boundary=1), dict(max_displacement=0), dict(max_displacement=-1),
           dict(max_displacement=np.nan), dict(max_displacement=np.inf), dict(max_displacement=1e60), dict(max_displacement=1e-60),
           dict(max_displacement="x"), dict(max_displacement=True)]
    for kw in bad:
        options = dict(dict(iterations=2), **kw)
        with pytest.raises(ValueError):
            mesh_smooth.check_options(**options)
        with pytest.raises(ValueError):
            mesh_smooth.smooth_mesh(v, None, f, **options)                     # a ValueError with or without a GPU
    for args in ((v[:, :2], None, f), (v, None, f[:, :2]), (v, np.zeros((3, 3), np.uint8), f), (v, None, 7)):
        with pytest.raises(ValueError):
            mesh_smooth.smooth_mesh(*args, 1)
    with pytest.raises(ValueError):
        mesh_smooth.smooth_mesh(v, None, f, 1, device="cpu")
    z = np.zeros((2, 4, 4), np.float32)
    for kw in (dict(smooth_iterations=-1), dict(smooth_iterations=1, smooth_lambda=0), dict(smooth_iterations=2, smooth_mu=1),
               dict(smooth_iterations=2, smooth_boundary="x"), dict(smooth_iterations=2, smooth_max_voxels=0)):
        with pytest.raises(ValueError):
            mesh.mesh_depth_maps(z, z, np.zeros((2, 2, 4, 4)), **kw)
    vol_options = dict(iterations=0)
    with pytest.raises(ValueError):
        mesh_smooth.check_options(**vol_options)


def test_the_three_command_lines_check_their_options(tmp_path):
    from mvsnet_amd import depthfusion, mesh, mesh_smooth
    src, out = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    a = mesh_smooth.parse_args(["--mesh", src, "--out", out, "--iterations", "5"])
    assert (a.iterations, a.lam, a.mu, a.boundary, a.max_displacement, a.force) == (5, 0.5, float(np.float32(-0.53)), "fixed", None, False)
    a = mesh_smooth.parse_args(["--mesh", src, "--out", out, "--iterations", "2", "--lambda", "0.25", "--mu", "0", "--boundary", "curve",
                                "--max_displacement", "0.5", "--force"])
    assert (a.iterations, a.lam, a.mu, a.boundary, a.max_displacement, a.force) == (2, 0.25, 0.0, "curve", 0.5, True)
    for extra in ([], ["--iterations", "0"], ["--iterations", "1001"], ["--iterations", "2", "--lambda", "0"],
                  ["--iterations", "2", "--lambda", "nan"], ["--iterations", "2", "--mu", "0.5"], ["--iterations", "2", "--boundary", "x"],
                  ["--iterations", "2", "--max_displacement", "0"], ["--iterations", "2", "--max_displacement", "inf"]):
        with pytest.raises(SystemExit):
            mesh_smooth.parse_args(["--mesh", src, "--out", out] + extra)
    open(out, "wb").close()                                                    # an existing output is refused before any GPU work
    with pytest.raises(SystemExit) as e:
        mesh_smooth.main(["--mesh", src, "--out", out, "--iterations", "1"])
    assert "--force" in str(e.value)
    a = mesh.parse_args(["--dense_folder", str(tmp_path)])                     # --smooth_iterations 0: nothing of it runs
    assert a.smooth_iterations == 0 and a.stages["smooth"] is None and mesh.stage_keywords(a.stages) == {}
    a = mesh.parse_args(["--dense_folder", str(tmp_path), "--smooth_iterations", "0", "--smooth_lambda", "0.3"])
    assert a.stages["smooth"] is None and mesh.stage_keywords(a.stages) == {}
    a = mesh.parse_args(["--dense_folder", str(tmp_path), "--smooth_iterations", "10", "--smooth_mu", "-0.4", "--smooth_max_voxels", "2"])
    assert mesh.stage_keywords(a.stages) == dict(smooth_iterations=10, smooth_lambda=0.5, smooth_mu=float(np.float32(-0.4)),
                                                 smooth_boundary="fixed", smooth_max_voxels=2.0)
    for bad in (["--smooth_iterations", "-1"], ["--smooth_iterations", "1001"], ["--smooth_iterations", "2", "--smooth_lambda", "2"],
                ["--smooth_iterations", "2", "--smooth_mu", "nan"], ["--smooth_iterations", "2", "--smooth_max_voxels", "0"],
                ["--smooth_iterations", "2", "--smooth_boundary", "x"]):
        with pytest.raises(SystemExit) as e:
            mesh.parse_args(["--dense_folder", str(tmp_path)] + bad)
        assert "smooth" in str(e.value) or e.value.code == 2                   # argparse's own exit for the choice
    for flag, value in (("iterations", "3"), ("lambda", "0.3"), ("mu", "-0.2"), ("boundary", "free"), ("max_voxels", "2")):
        with pytest.raises(SystemExit) as e:
            depthfusion.main(["--dense_folder", str(tmp_path / "none"), "--fusion", "hip", "--mesh_smooth_" + flag, value])
        assert "--mesh_smooth_%s needs --mesh" % flag in str(e.value)
    with pytest.raises(SystemExit) as e:
        depthfusion.main(["--dense_folder", str(tmp_path / "none"), "--fusion", "hip", "--mesh", "--mesh_smooth_iterations", "2000"])
    assert "--mesh_smooth_iterations" in str(e.value)
    with pytest.raises(SystemExit) as e:
        depthfusion.main(["--dense_folder", str(tmp_path / "none"), "--mesh", "--mesh_smooth_iterations", "2"])
    assert "--mesh needs --fusion hip" in str(e.value)
    assert not (tmp_path / "none").exists()


# ------------------------------------------------------------------------------------------------ the library, without a GPU

def test_names_and_their_place_in_the_signatures():
    from mvsnet_amd import _lib, build
    assert "mesh_smooth.hip" in build.SOURCES
    names = list(_lib.SIGNATURES)
    smooth = [name for name in names if name.startswith("mvs_mesh_smooth")]
    assert sorted(smooth) == sorted(["mvs_mesh_smooth_workspace_bytes", "mvs_mesh_smooth_edges_i64", "mvs_mesh_smooth_heads_i64",
                                     "mvs_mesh_smooth_rows_i32", "mvs_mesh_smooth_step_f32"])
    assert all(names.index(name) < names.index("mvs_fusion_workspace_bytes") for name in smooth)


def test_library_checks_arguments_before_any_gpu_call(lib_built):
    """Argument validation happens before the first HIP call, so the codes are testable without a GPU: the pointers below are
    host buffers that a kernel must never see."""
    from mvsnet_amd import _lib
    h = _lib.load()
    assert h.mvs_abi_version() == 1
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.c_void_p(p.value + 4096)
    big, nan, inf = 2 ** 31, float("nan"), float("inf")
    most = (2 ** 31 - 1) // 6
    wsb = h.mvs_mesh_smooth_workspace_bytes
    assert wsb(0, 0) == 256 and wsb(5, 9) == 256 and wsb(big - 1, most) == 256
    assert wsb(-1, 0) == 0 and wsb(0, -1) == 0 and wsb(big, 1) == 0 and wsb(1, most + 1) == 0
    edges = lambda v=p, M=8, f=p, F=4, k=p, ws=p, n=256: h.mvs_mesh_smooth_edges_i64(v, M, f, F, k, ws, n, None)
    for kw in (dict(v=None), dict(f=None), dict(k=None), dict(ws=None), dict(M=-1), dict(F=-1)):
        assert edges(**kw) == -1, kw
    assert edges(M=big) == -2 and edges(F=most + 1) == -2 and edges(n=255) == -3
    heads = lambda sk=p, F=4, head=p, ws=p, n=256: h.mvs_mesh_smooth_heads_i64(sk, F, head, ws, n, None)
    for kw in (dict(sk=None), dict(head=None), dict(ws=None), dict(F=-1)):
        assert heads(**kw) == -1, kw
    assert heads(F=most + 1) == -2 and heads(n=255) == -3
    rows = lambda sk=p, head=p, rank=p, M=8, F=4, mode=0, nb=p, rs=p, vc=p, ws=p, n=256: h.mvs_mesh_smooth_rows_i32(
        sk, head, rank, M, F, mode, nb, rs, vc, ws, n, None)
    for kw in (dict(sk=None), dict(head=None), dict(rank=None), dict(nb=None), dict(rs=None), dict(vc=None), dict(ws=None), dict(M=-1),
               dict(F=-1), dict(mode=3), dict(mode=-1)):
        assert rows(**kw) == -1, kw
    assert rows(M=big) == -2 and rows(F=most + 1) == -2 and rows(n=255) == -3
    step = lambda X=p, V0=p, rs=p, nb=p, vc=p, M=8, N=24, row=3, f=0.5, r=-1.0, Y=q: h.mvs_mesh_smooth_step_f32(
        X, V0, rs, nb, vc, M, N, row, f, r, Y, None)
    for kw in (dict(X=None), dict(V0=None), dict(rs=None), dict(nb=None), dict(vc=None), dict(Y=None), dict(Y=p), dict(M=-1), dict(N=-1),
               dict(row=2), dict(row=5), dict(f=nan), dict(f=inf), dict(r=nan), dict(r=inf),
               dict(row=4, X=ctypes.c_void_p(p.value + 4))):
        assert step(**kw) == -1, kw
    assert step(M=big) == -2 and step(N=big) == -2 and step(M=0, X=None, V0=None, rs=None, nb=None, vc=None, Y=None) == 0
