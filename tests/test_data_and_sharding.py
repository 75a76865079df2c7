"""CPU tests of the host logic around the hot path: session loader, output
writers, and the world_size-2 sharding path over gloo."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


from _helpers import make_session  # noqa: E402


def test_scale_image_kats():
    from mvsnet_amd.mvs_data_generation import scale_image
    ramp = np.arange(8, dtype=np.float32)[None, :].repeat(4, 0)           # value = x
    half = scale_image(ramp, 0.5)                                          # src = 2*dst + 0.5
    assert half.shape == (2, 4)
    np.testing.assert_allclose(half[0], [0.5, 2.5, 4.5, 6.5])
    dbl = scale_image(ramp, 2.0)                                           # src = dst/2 - 0.25, edges clamp
    assert dbl.shape == (8, 16)
    np.testing.assert_allclose(dbl[0, :4], [0.0, 0.25, 0.75, 1.25])
    np.testing.assert_allclose(dbl[0, -1], 7.0)
    u8 = scale_image((ramp * 30).astype(np.uint8), 0.5)
    assert u8.dtype == np.uint8 and list(u8[0]) == [15, 75, 135, 195]
    near = scale_image(ramp, 0.5, "nearest")
    assert list(near[0]) == [0, 2, 4, 6]
    col = scale_image(np.zeros((6, 10, 3), np.uint8), 0.25)
    assert col.shape == (2, 2, 3)                                          # round(1.5) = 2, round(2.5) = 2


def test_crop_center_and_camera_scaling():
    from mvsnet_amd import mvs_data_generation as G
    img = np.arange(10 * 12 * 3, dtype=np.float32).reshape(10, 12, 3)
    cam = np.zeros((2, 4, 4)); cam[1, 0, 0] = cam[1, 1, 1] = 100; cam[1, 0, 2] = 6; cam[1, 1, 2] = 5
    imgs, cams = G.crop_mvs_input([img], [cam], width=8, height=8, base_image_size=8)
    assert imgs[0].shape == (8, 8, 3)
    assert np.array_equal(imgs[0], img[1:9, 2:10])
    assert cams[0][1, 0, 2] == 4 and cams[0][1, 1, 2] == 4
    c2 = G.scale_camera(cam, 0.25)
    assert c2[1, 0, 0] == 25 and c2[1, 0, 2] == 1.5 and c2[1, 1, 2] == 1.25
    z = G.center_image(img)
    np.testing.assert_allclose(z.mean(axis=(0, 1)), 0, atol=1e-5)
    np.testing.assert_allclose(z.std(axis=(0, 1)), 1, atol=1e-5)


def test_cluster_generator_on_synthetic_session(tmp_path):
    from mvsnet_amd.mvs_data_generation import ClusterGenerator
    sess = make_session(str(tmp_path / "sess"))
    gen = ClusterGenerator(sess, view_num=3, image_width=32, image_height=32, depth_num=8,
                           interval_scale=1.0, base_image_size=8, output_scale=0.25)
    assert len(gen) == 3                                   # image 3 has no covisible views -> skipped
    items = list(gen)
    out_images, in_images, out_cams, full_cams, idx = items[0]
    assert idx == 0
    assert in_images.shape == (3, 32, 32, 3) and in_images.dtype == np.float32
    assert out_images.shape == (3, 8, 8, 3)
    assert out_cams.shape == (3, 2, 4, 4) and full_cams.shape == (3, 2, 4, 4)
    # rescale = max(32/48, 32/64) = 2/3 -> 32 x 43 -> centre crop 32 x 32; intrinsics follow
    np.testing.assert_allclose(full_cams[0, 1, 0, 0], 60.0 * 2 / 3)
    np.testing.assert_allclose(out_cams[0, 1, 0, 0], 60.0 * 2 / 3 * 0.25)
    np.testing.assert_allclose(out_cams[0, 1, 3], [400.0, 500.0 / 7, 8, 900.0])
    np.testing.assert_allclose(out_cams[1, 0, 0, 3], 50.0)                # metres -> mm
    # a cluster with one covisible view is padded with copies of the reference
    c = gen.clusters[0]
    c2 = type(c)(c.session_dir, 0, [2], 400.0, 900.0, 3)
    assert c2.indices == [0, 2, 0]


def test_write_output_slice_files(tmp_path):
    from mvsnet_amd import predictlib as pl, preprocess as pp
    depth = np.linspace(425, 900, 12, dtype=np.float32).reshape(1, 3, 4, 1)
    prob = np.linspace(0, 1, 12, dtype=np.float32).reshape(1, 3, 4, 1)
    img = np.zeros((3, 4, 3), np.float32); img[..., 0] = 255            # blue in BGR
    cam = np.zeros((2, 4, 4)); cam[0] = np.eye(4); cam[1, :3, :3] = np.eye(3)
    out = pl.setup_output_dir(str(tmp_path), None)
    assert out == os.path.join(str(tmp_path), "depths_mvsnet")
    pl.write_output_slice(out, depth, prob, img, cam, np.array([7]))
    names = sorted(os.listdir(out))
    assert names == ["7.jpg", "7.txt", "7_depth.png", "7_init.pfm", "7_prob.pfm", "7_prob.png"]
    assert np.array_equal(pp.load_pfm(os.path.join(out, "7_init.pfm")), depth[0, :, :, 0])
    from PIL import Image
    d16 = np.asarray(Image.open(os.path.join(out, "7_depth.png")))
    assert d16.dtype == np.uint16 and d16[0, 0] == 425 and d16[-1, -1] == 900
    p16 = np.asarray(Image.open(os.path.join(out, "7_prob.png")))
    assert p16[0, 0] == 0 and p16[-1, -1] == 65535
    rgb = np.asarray(Image.open(os.path.join(out, "7.jpg")))
    assert rgb[0, 0, 2] > 200 and rgb[0, 0, 0] < 50                      # written as RGB


def test_shard_indices_cover_everything_once():
    from mvsnet_amd.shard import shard_indices
    for n in (0, 1, 7, 1078):
        for world in (1, 2, 3, 8):
            parts = [shard_indices(n, r, world) for r in range(world)]
            flat = sorted(i for p in parts for i in p)
            assert flat == list(range(n))
            assert max(len(p) for p in parts) - min(len(p) for p in parts) <= 1
    with pytest.raises(ValueError):
        shard_indices(4, 2, 2)


_WORKER = r"""
import os, sys, json
sys.path.insert(0, %(root)r)
from mvsnet_amd import shard as sh
dist = sh.init_process_group("gloo")
rank, local, world = sh.rank_world()
items = list(range(11))
mine = sh.shard(items, rank, world)
counts = sh.gather_counts(dist, len(mine))
import torch
t = torch.zeros(11, dtype=torch.int64); t[mine] = 1
dist.all_reduce(t)                      # test-only check that the shards tile the list
dist.barrier()
if rank == 0:
    print(json.dumps({"counts": counts, "cover": t.tolist(), "world": world}))
dist.destroy_process_group()
"""


def test_world_size_2_sharding_over_gloo(tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", WORLD_SIZE="2")
    from _helpers import run_ranks
    outs = run_ranks(_WORKER % {"root": ROOT}, env, world=2, timeout=180)
    assert all(rc == 0 for rc, _o, _e in outs), outs
    res = json.loads(outs[0][1].strip().splitlines()[-1])
    assert res["world"] == 2 and res["counts"] == [6.0, 5.0]
    assert res["cover"] == [1] * 11


def make_pair_project(path, n_images=3, h=48, w=64, seed=1):
    """A tiny project folder in the upstream MVSNet format (images/, cams/, pair.txt)."""
    from PIL import Image
    rs = np.random.RandomState(seed)
    os.makedirs(os.path.join(path, "images")); os.makedirs(os.path.join(path, "cams"))
    for i in range(n_images):
        Image.fromarray(rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).save(
            os.path.join(path, "images", "%08d.jpg" % i), quality=95)
        ext = np.eye(4); ext[0, 3] = -30.0 * i
        K = np.array([[60.0, 0, w / 2.0], [0, 60.0, h / 2.0], [0, 0, 1.0]])
        with open(os.path.join(path, "cams", "%08d_cam.txt" % i), "w") as f:
            f.write("extrinsic\n" + "\n".join(" ".join(str(v) for v in row) for row in ext) + "\n\n")
            f.write("intrinsic\n" + "\n".join(" ".join(str(v) for v in row) for row in K) + "\n\n")
            f.write("425.0 2.5\n")
    with open(os.path.join(path, "pair.txt"), "w") as f:
        f.write("%d\n" % n_images)
        for i in range(n_images):
            others = [j for j in range(n_images) if j != i]
            f.write("%d\n%d %s\n" % (i, len(others), " ".join("%d %.1f" % (j, 100.0 - j) for j in others)))
    return path


def test_upstream_pair_txt_project(tmp_path):
    from mvsnet_amd.mvs_data_generation import make_generator, gen_pipeline_mvs_list, PairClusterGenerator
    proj = make_pair_project(str(tmp_path / "proj"))
    lst = gen_pipeline_mvs_list(proj, view_num=3)
    assert [r for r, _ in lst] == [0, 1, 2]
    assert lst[0][1][0].endswith("images/00000000.jpg") and lst[0][1][3].endswith("cams/00000001_cam.txt")
    gen = make_generator(proj, 5, 32, 32, 16, 1.06, 8, output_scale=0.25)
    assert isinstance(gen, PairClusterGenerator) and len(gen) == 3
    out_images, in_images, out_cams, full_cams, idx = next(iter(gen))
    assert idx == 0 and in_images.shape == (5, 32, 32, 3)               # 2 sources + 2 reference pads
    assert np.array_equal(in_images[3], in_images[0]) and np.array_equal(out_cams[4], out_cams[0])
    np.testing.assert_allclose(out_cams[0, 1, 3], [425.0, 2.65, 16, 425.0 + 2.65 * 16])   # 29-word cams + max_d
    np.testing.assert_allclose(out_cams[1, 0, 0, 3], -30.0)


def test_semilite_has_the_reference_runtime_channel_counts():
    """network.py:75-76 writes `self.base_divisor = 4/3` in a Python 2.7 module with no `division` import
    (network.py:9): integer 1 at run time, so 'semilite' networks are 'normal'-sized (base_filter 8, 32-channel
    features) and only the ConvGRU filters are halved (model.py:641-645)."""
    from mvsnet_amd import synthetic as S
    assert S.base_filter("semilite") == 8 == S.base_filter("normal")
    assert S.make_workload("toy", "semilite").channels == 32
    assert S.gru_filters("semilite") == (8, 2, 1) and S.gru_filters("normal") == (16, 4, 2)
    assert S.base_filter("semilite-py3") == 6 and S.base_filter("lite") == 4 and S.base_filter("fat") == 16
    a = S.make_regnet_params("semilite", seed=1)
    b = S.make_regnet_params("normal", seed=1)
    assert all(a[k]["w"].shape == b[k]["w"].shape for k in b)


def test_session_writer_and_per_image_cache_equal_the_per_cluster_path(tmp_path):
    """synthetic.write_session produces a session the generator reads (N = 5, D = 192 from the depth range), and the cached
    inference path of ClusterGenerator (decode / rescale / crop once per IMAGE, round 3) returns exactly what the reference's
    per-cluster sequence returns (cluster_generator.py:234-286: load all views, scale, crop, centre, output-scale) -- also
    when the images need rescaling and cropping, and with the standardisation left to the caller (uint8 out)."""
    from mvsnet_amd import synthetic as S
    from mvsnet_amd import mvs_data_generation as G
    sess = S.write_session(str(tmp_path / "s"), n_images=6, height=100, width=132, view_num=5, depth_num=192)
    gen = G.make_generator(sess, 5, 128, 96, 192, 1.0, 8, mode="inference", output_scale=0.25)
    assert len(gen.clusters) == 6
    for ci in (0, 3, 5):
        c = gen.clusters[ci]
        got = gen.prepare(c)
        c2 = G.make_generator(sess, 5, 128, 96, 192, 1.0, 8, mode="inference", output_scale=0.25).clusters[ci]
        images, cams = c2.images(), c2.cameras()
        images, cams = G.scale_mvs_input(images, cams, scale=c2.rescale)
        ci_, cc_ = G.crop_mvs_input(images, cams, 128, 96, 8)
        oi, oc = G.scale_mvs_input(ci_, cc_, scale=0.25)
        want = (np.stack(oi), np.stack([G.center_image(i) for i in ci_]), np.stack(oc), np.stack(cc_), c2.ref_index)
        assert c.rescale == c2.rescale and len(c.indices) == 5
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        raw = gen.prepare(c, center=False)
        assert raw[1].dtype == np.uint8 and np.array_equal(raw[1], np.stack(ci_))
        assert got[2][0, 1, 3, 2] == 192 and abs(got[2][0, 1, 3, 1] - 2.65) < 1e-6
    # second request of a cluster: served from the cache, same arrays
    again = gen.prepare(gen.clusters[0])
    assert np.array_equal(again[1], gen.prepare(gen.clusters[0])[1])


def test_launch_ranks_starts_the_ranks_and_returns_their_exit_code(tmp_path):
    """shard.launch_ranks (what `bench.py --gpus N` / `inference --gpus N` call when started without a launcher): N ranks
    under torch.distributed.run on 127.0.0.1 and a free port; exit code 0 when all ranks succeed, non-zero when one fails."""
    from mvsnet_amd.shard import launch_ranks
    ok = tmp_path / "ok.py"
    ok.write_text("import os, sys\nsys.path.insert(0, %r)\nfrom mvsnet_amd import shard as sh\ndist = sh.init_process_group('gloo')\n"
                  "r, l, w = sh.rank_world()\nassert w == 2\nopen(os.path.join(%r, 'rank%%d' %% r), 'w').write(str(sh.gather_counts(dist, r + 1)))\n"
                  "dist.destroy_process_group()\n" % (ROOT, str(tmp_path)))
    assert launch_ranks([str(ok)], 2) == 0
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("rank")) == ["rank0", "rank1"]
    assert open(tmp_path / "rank0").read() == "[1.0, 2.0]"
    bad = tmp_path / "bad.py"
    bad.write_text("import os, sys\nsys.exit(3 if os.environ['RANK'] == '1' else 0)\n")
    assert launch_ranks([str(bad)], 2) != 0


def test_eight_ranks_plumbing_over_gloo(tmp_path):
    """SURVEY 8e at the node's size: 8 ranks started by shard.launch_ranks (free port, 127.0.0.1), gloo group, round-robin shard
    of config 4's 1078 reference views (22 scans x 49 views), the per-rank gathers and object gather bench.py's record uses,
    8 ranks x 3 processes per GPU folded onto the first 8 devices (MVS_GPUS), and the exit code of ONE failing rank among 8.
    (The GPU box admits at most 6 processes on its card, so the 8-rank case is rehearsed here on the CPU; the GPU suite runs
    bench.py with 4 ranks on one card, tests/test_gpu_pipeline.py.)"""
    from mvsnet_amd.shard import launch_ranks
    ok = tmp_path / "ok8.py"
    ok.write_text(
        "import os, sys, json\nsys.path.insert(0, %r)\nfrom mvsnet_amd import shard as sh\nimport torch\n"
        "dist = sh.init_process_group('gloo')\nr, l, w = sh.rank_world()\nassert w == 8 and l == r\n"
        "mine = sh.shard(list(range(1078)), r, w)\ncounts = sh.gather_counts(dist, len(mine))\n"
        "t = torch.tensor([0.5 + 0.01 * r], dtype=torch.float64)\ndist.all_reduce(t, op=dist.ReduceOp.MAX)\n"
        "devs = [None] * w\ndist.all_gather_object(devs, {'rank': r, 'device_index': sh.device_index_of(l, 8)})\ndist.barrier()\n"
        "if r == 0:\n    open(os.path.join(%r, 'rec.json'), 'w').write(json.dumps({'counts': counts, 'max': float(t), 'devs': devs}))\n"
        "dist.destroy_process_group()\n" % (ROOT, str(tmp_path)))
    assert launch_ranks([str(ok)], 8) == 0
    rec = json.loads(open(tmp_path / "rec.json").read())
    assert rec["counts"] == [135.0] * 6 + [134.0] * 2 and sum(rec["counts"]) == 1078        # ~135 reference views per GPU
    assert abs(rec["max"] - 0.57) < 1e-12
    assert [d["device_index"] for d in rec["devs"]] == list(range(8)) and [d["rank"] for d in rec["devs"]] == list(range(8))
    bad = tmp_path / "bad8.py"
    bad.write_text("import os, sys, time\ntime.sleep(0.2)\nsys.exit(3 if os.environ['RANK'] == '5' else 0)\n")
    assert launch_ranks([str(bad)], 8) != 0


def test_processes_per_gpu_fold_onto_the_requested_gpus_not_onto_all_visible(monkeypatch):
    """`--gpus G --procs_per_gpu P` starts G x P ranks; rank r drives GPU r mod G whatever the node shows (round 3
    took r mod device_count: `--gpus 1 --procs_per_gpu 3` on an 8-GPU node spread over GPUs 0, 1, 2)."""
    from mvsnet_amd import shard as sh
    monkeypatch.delenv("MVS_ALLOW_SHARED_GPU", raising=False)
    monkeypatch.setenv("MVS_GPUS", "1")
    assert [sh.device_index_of(r, 8) for r in range(3)] == [0, 0, 0]
    monkeypatch.setenv("MVS_GPUS", "2")
    assert [sh.device_index_of(r, 8) for r in range(6)] == [0, 1, 0, 1, 0, 1]
    monkeypatch.delenv("MVS_GPUS")
    assert [sh.device_index_of(r, 8) for r in range(8)] == list(range(8))
    assert sh.device_index_of(3, 1) == 3                                 # no folding without the rehearsal switch: bind_device refuses
    monkeypatch.setenv("MVS_ALLOW_SHARED_GPU", "1")
    assert [sh.device_index_of(r, 1) for r in range(8)] == [0] * 8
    # launch_ranks hands MVS_GPUS to its ranks only when ranks share GPUs
    import subprocess
    seen = {}
    monkeypatch.setattr(subprocess, "call", lambda cmd, env=None: seen.update(env=env, cmd=cmd) or 0)
    monkeypatch.delenv("MVS_GPUS", raising=False)
    assert sh.launch_ranks(["x.py"], 6, gpus=2) == 0 and seen["env"]["MVS_GPUS"] == "2" and "6" in seen["cmd"]
    assert sh.launch_ranks(["x.py"], 8, gpus=8) == 0 and "MVS_GPUS" not in seen["env"]
    assert sh.launch_ranks(["x.py"], 8) == 0 and "MVS_GPUS" not in seen["env"]


def test_feature_cache_never_evicts_a_key_of_the_group_in_hand():
    """the per-image feature cache is a true LRU whose limit may be SMALLER than one group's key set; keys that were
    hits when the group was formed stay readable until the next group (round 3: FIFO eviction during insertion -> KeyError)."""
    from mvsnet_amd.inference import FeatureCache
    calls = []

    def tower(imgs):
        calls.append(list(imgs))
        return ["F(%s)" % i for i in imgs]
    c = FeatureCache(limit=4)
    c.fill([(k, "img%d" % k) for k in (0, 1, 2, 3)], tower)
    assert calls == [["img0", "img1", "img2", "img3"]] and c.get([3, 0]) == ["F(img3)", "F(img0)"]
    # group 2: hits 0 and 1 (old entries, first in line for eviction), misses 4..8 -- more keys than the limit
    c.fill([(k, "img%d" % k) for k in (0, 1, 4, 5, 6, 7, 8, 0, 4)], tower)
    assert calls[1] == ["img4", "img5", "img6", "img7", "img8"]                       # one tower pass, misses only, no repeats
    assert c.get([0, 1, 4, 5, 6, 7, 8]) == ["F(img%d)" % k for k in (0, 1, 4, 5, 6, 7, 8)]
    assert len(c.entries) == 4 and list(c.entries) == [5, 6, 7, 8]                    # newest kept
    # LRU, not FIFO: a hit refreshes the entry
    c.fill([(5, "img5")], tower)
    c.fill([(9, "img9")], tower)
    assert list(c.entries) == [7, 8, 5, 9] and c.hits == 3 and c.misses == 10
    with pytest.raises(KeyError):
        c.get([6])                                                                     # not part of the group in hand


def test_a_recurrent_sweep_takes_views_of_one_feature_shape_and_depth_count():
    """The GRU batcher sends the pending views off before a view of another feature shape or depth count joins them."""
    from mvsnet_amd.inference import _starts_new_sweep
    pending = [(np.zeros((5, 128, 160, 32), np.float32), "cams", 192)]
    assert not _starts_new_sweep([], (5, 96, 128, 32), 96)
    assert not _starts_new_sweep(pending, (5, 128, 160, 32), 192)
    assert _starts_new_sweep(pending, (5, 96, 128, 32), 192)
    assert _starts_new_sweep(pending, (5, 128, 160, 32), 96)


def test_host_worker_processes_equal_the_in_process_loader_and_writer(tmp_path):
    """mvsnet_amd/host_pool.py (round 4): the per-image part of the loader (decode -> scale-to-cover -> centre-crop -> output
    scale) and write_output_slice run in spawned worker PROCESSES; a cluster assembled by inference.SessionLoader equals
    ClusterGenerator.prepare(c, center=False) array for array, the six files a worker writes equal the in-process writer's
    byte for byte, the workers see no GPU and import nothing of the application's __main__."""
    import numpy as np
    from mvsnet_amd import host_pool, mvs_data_generation as G, predictlib as pl, synthetic as S
    from mvsnet_amd.inference import SessionLoader
    sess = S.write_session(str(tmp_path / "s"), n_images=7, height=100, width=132, view_num=5, depth_num=192)
    mk = lambda: G.make_generator(sess, 5, 128, 96, 192, 1.0, 8, mode="inference", output_scale=0.25)
    gen = mk()
    pool = host_pool.get_pool(2)
    assert pool.workers == 2 and len(pool.pids) >= 1 and os.getpid() not in pool.pids
    sl = SessionLoader(gen, pool)
    handles = [sl.submit(c) for c in gen.clusters]                       # 7 images requested once each, 35 uses
    want = None
    for c, h in zip(gen.clusters, handles):
        got = sl.result(h)
        gen2 = mk()
        c2 = [x for x in gen2.clusters if x.ref_index == c.ref_index][0]
        want = gen2.prepare(c2, center=False)
        assert isinstance(got[0], list) and got[1][0].dtype == np.uint8
        assert np.array_equal(np.stack(got[0]), want[0]) and np.array_equal(np.stack(got[1]), want[1])
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and got[4] == want[4]
        assert c.rescale == c2.rescale and tuple(c.original_image_shape) == tuple(c2.original_image_shape)
    assert len(sl.images) == 7 and sl.load_seconds > 0
    rs = np.random.RandomState(0)
    depth = (rs.rand(24, 32) * 500 + 425).astype(np.float32)
    prob = rs.rand(24, 32).astype(np.float32)
    o1, o2 = str(tmp_path / "o1"), str(tmp_path / "o2")
    os.makedirs(o1); os.makedirs(o2)
    assert pool.write_outputs(o1, depth, prob, want[0][0], want[2][0], 7).result() > 0
    pl.write_output_slice(o2, depth, prob, want[0][0], want[2][0], 7)
    assert sorted(os.listdir(o1)) == sorted(os.listdir(o2)) == ["7.jpg", "7.txt", "7_depth.png", "7_init.pfm", "7_prob.pfm", "7_prob.png"]
    for fn in os.listdir(o2):
        assert open(os.path.join(o1, fn), "rb").read() == open(os.path.join(o2, fn), "rb").read(), fn
    # a failing task surfaces in the parent as the worker's exception, and the slot it held is free again
    bad = pool.load_image(str(tmp_path / "missing.jpg"), 1.0, 128, 96, 8, 0.25)
    with pytest.raises(FileNotFoundError):
        bad.result()
    assert len(pool.free) == pool.slots
    # the workers were started without devices and without the application's main module
    env = pool.ex.submit(_worker_probe).result()
    assert env["hip"] == "" and env["worker"] == "1" and env["main_file"] is None and env["torch"] is False
    assert host_pool.get_pool(0) is None                                  # threads only
    # a /dev/shm without room for a slot ring (containers often give it 64 MB): images come back through the pool's pipe, same arrays
    import collections
    small = host_pool.HostPool(1, slots=8)
    try:
        fake = collections.namedtuple("vfs", "f_bavail f_frsize")(16, 4096)
        real = os.statvfs
        os.statvfs = lambda path_: fake if path_ == "/dev/shm" else real(path_)
        try:
            img = os.path.join(sess, "images", "3.jpg")
            cr, oi, shape, sec = small.load_image(img, 1.0, 128, 96, 8, 0.25).result()
        finally:
            os.statvfs = real
        assert small.shm is None and small.slot_bytes == -1
        want_cr, want_oi, want_shape = host_pool.prepare_image(img, 1.0, 128, 96, 8, 0.25)
        assert np.array_equal(cr, want_cr) and np.array_equal(oi, want_oi) and tuple(shape) == tuple(want_shape) and sec > 0
    finally:
        small.close()


def _worker_probe():
    import sys
    return {"hip": os.environ.get("HIP_VISIBLE_DEVICES"), "worker": os.environ.get("MVS_HOST_WORKER"),
            "main_file": getattr(sys.modules["__main__"], "__file__", None), "torch": "torch" in sys.modules}


def test_host_pool_shares_dev_shm_between_the_ranks_of_a_node(monkeypatch):
    """the image-slot ring of host_pool takes a quarter of what /dev/shm has free -- per NODE: with
    LOCAL_WORLD_SIZE ranks starting together each may reserve 1/LOCAL_WORLD_SIZE of that quarter, so eight ranks against a
    64 MB tmpfs ask for 16 MB in total, not 128."""
    from mvsnet_amd import host_pool

    class FakeVfs:
        f_bavail, f_frsize = 64 * 256, 4096                   # 64 MB free
    fake = lambda path: FakeVfs()
    monkeypatch.delenv("LOCAL_WORLD_SIZE", raising=False)
    assert host_pool.shm_room(fake) == 16 * 2 ** 20
    monkeypatch.setenv("LOCAL_WORLD_SIZE", "8")
    rooms = [host_pool.shm_room(fake) for _ in range(8)]      # eight pools, one per rank
    assert all(r == 2 * 2 ** 20 for r in rooms) and sum(rooms) <= 64 * 2 ** 20 // 4
    # a 640 x 512 session needs 0.94 MB per slot: 2 slots < the pool's minimum of 4 -> it goes back to the pipe instead of SIGBUS
    assert rooms[0] // (640 * 512 * 3) < 4


def test_host_pool_starts_every_worker_without_a_gpu_and_with_an_empty_main():
    """all `workers` processes must be started inside the window in which the parent hides the GPU and its __main__
    (ProcessPoolExecutor starts workers on demand); the pool's pid list is the executor's own process table."""
    from mvsnet_amd import host_pool
    pool = host_pool.HostPool(3, slots=8)
    try:
        assert len(pool.pids) == 3 == len(pool.ex._processes)
        envs = [pool.ex.submit(_worker_env).result() for _ in range(12)]
        assert {e[0] for e in envs} <= set(pool.pids)
        assert all(e[1] == "" and e[2] == "1" and e[3] is False for e in envs)       # no GPU, marked as a worker, no application __main__
    finally:
        pool.ex.shutdown(wait=True)


def _worker_env():
    import sys
    main = sys.modules.get("__main__")
    return (os.getpid(), os.environ.get("HIP_VISIBLE_DEVICES"), os.environ.get("MVS_HOST_WORKER"), hasattr(main, "test_host_pool_starts_every_worker_without_a_gpu_and_with_an_empty_main"))
