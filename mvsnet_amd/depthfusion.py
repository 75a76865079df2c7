"""Post-processing hand-off to Gipuma / fusibile, mirroring mvsnet/depthfusion.py:

    python -m mvsnet_amd.depthfusion --dense_folder <dir> [--fusibile_exe_path <exe>]
        [--prob_threshold 0.8] [--disp_threshold 0.25] [--num_consistent 3]

1. probability filter: <idx>_init.pfm with depth 0 where <idx>_prob.pfm < threshold ->
   <idx>_prob_filtered.pfm (depthfusion.py:171-189);
2. Gipuma layout under <dense_folder>/points_mvsnet: cams/<name>.P (3x4 projection K[R|t]),
   images/<name>, 2333__<idx>/disp.dmb + normals.dmb (constant 1/sqrt(3) normals masked by depth > 0)
   (depthfusion.py:28-168);
3. the external `fusibile` binary is run when it exists (depthfusion.py:192-213); it is not part of
   this package, so without it the converted folder is the result.
With --fusion hip, steps 2 and 3 are replaced by this project's own geometric-consistency fusion on the GPU
(mvsnet_amd.fusion: a HIP kernel, not bit-compatible with fusibile), which writes
points_mvsnet/consistencyCheck-<YYYYmmdd-HHMMSS>/final3d_model.ply, the path the reference's scripts look for:
    python -m mvsnet_amd.depthfusion --dense_folder <dir> --fusion hip [--reproj_threshold 1.0]
        [--depth_rel_threshold 0.01] [--no_dedupe] [--fusion_sources {all,listed}] [--mesh]
        [--mesh_min_component_faces 0] [--mesh_min_component_extent 0] [--mesh_keep_largest 0] [--mesh_simplify_voxels S]
        [--mesh_smooth_iterations N [--mesh_smooth_lambda 0.5] [--mesh_smooth_mu -0.53] [--mesh_smooth_boundary fixed|curve|free]
         [--mesh_smooth_max_voxels 1]]
        [--mesh_recolour [--mesh_recolour_min_cos 0.2] [--mesh_recolour_angle_power 2] [--mesh_recolour_occlusion_rel 0.01]]
        [--eval_gt G.ply [--eval_max_dist 20] [--eval_thresholds 0.5,1,2] [--mesh_eval_spacing s]]
        [--normals] [--normal_angle_threshold DEG] [--jump_threshold 0.05] [--write_normal_maps]
--normals estimates surface normals from the depth maps on the GPU and writes the PLY as x y z nx ny nz red green blue
(fusibile's vertex layout); --normal_angle_threshold (implies --normals) also rejects pairs whose normals differ by more;
--write_normal_maps writes depths_mvsnet/<idx>_normal.pfm (colour PFM, camera frame).  The Gipuma hand-off keeps the
reference's constant fake normals.  And, with --eval_gt, evaluates that cloud against a ground-truth PLY on the GPU (mvsnet_amd.evaluate) into metrics.json beside it.
File formats are byte-compatible with the reference's writers (.dmb: int32 header 1,H,W,C +
float32 data in the reference's element order).
"""
from __future__ import annotations

import argparse
import glob
import os
import shutil
import struct
import subprocess

import numpy as np

from .preprocess import load_cam, load_pfm, write_pfm


def read_gipuma_dmb(path):
    """depthfusion.py:28-40: header (type, H, W, C) then float32 in column-major (W,H,C) order."""
    with open(path, "rb") as f:
        _type, height, width, channel = struct.unpack("<iiii", f.read(16))
        array = np.frombuffer(f.read(), np.float32)
    array = array.reshape((width, height, channel), order="F")
    return np.transpose(array, (1, 0, 2)).squeeze()


def write_gipuma_dmb(path, image):
    """depthfusion.py:43-64 (3-channel images are stored plane by plane, as the reference does)."""
    image = np.asarray(image)
    height, width = image.shape[0], image.shape[1]
    channels = image.shape[2] if image.ndim == 3 else 1
    if image.ndim == 3:
        image = np.transpose(image, (2, 0, 1)).squeeze()
    with open(path, "wb") as f:
        f.write(struct.pack("<iiii", 1, height, width, channels))
        np.ascontiguousarray(image).tofile(f)


def mvsnet_to_gipuma_dmb(in_path, out_path):
    write_gipuma_dmb(out_path, load_pfm(in_path))


def mvsnet_to_gipuma_cam(in_path, out_path):
    """depthfusion.py:76-99: P = K_4x4(last row zeroed) @ E, first three rows, str() formatted."""
    cam = load_cam(in_path)
    extrinsic = cam[0]
    intrinsic = cam[1].copy()
    intrinsic[3, :] = 0
    projection = np.matmul(intrinsic, extrinsic)[0:3]
    with open(out_path, "w") as f:
        for i in range(3):
            for j in range(4):
                f.write(str(projection[i][j]) + " ")
            f.write("\n")
        f.write("\n")


def fake_colmap_normal(in_depth_path, out_normal_path):
    """depthfusion.py:102-123."""
    depth = read_gipuma_dmb(in_depth_path)
    normal = np.ones(depth.shape + (3,), dtype=depth.dtype) / 1.732050808
    mask = np.float32(depth > 0)[..., None]
    write_gipuma_dmb(out_normal_path, np.float32(normal * mask))


def _depth_image_names(depth_folder):
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(depth_folder, "*.jpg")))


def probability_filter(dense_folder, prob_threshold):
    """depthfusion.py:171-189."""
    depth_folder = os.path.join(dense_folder, "depths_mvsnet")
    for name in _depth_image_names(depth_folder):
        prefix = os.path.splitext(name)[0]
        depth = load_pfm(os.path.join(depth_folder, prefix + "_init.pfm")).copy()
        prob = load_pfm(os.path.join(depth_folder, prefix + "_prob.pfm"))
        depth[prob < prob_threshold] = 0
        write_pfm(os.path.join(depth_folder, prefix + "_prob_filtered.pfm"), depth)


def mvsnet_to_gipuma(dense_folder, gipuma_point_folder):
    """depthfusion.py:126-168."""
    depth_folder = os.path.join(dense_folder, "depths_mvsnet")
    names = _depth_image_names(depth_folder)
    cam_folder = os.path.join(gipuma_point_folder, "cams")
    image_folder = os.path.join(gipuma_point_folder, "images")
    for d in (gipuma_point_folder, cam_folder, image_folder):
        os.makedirs(d, exist_ok=True)
    for name in names:
        prefix = os.path.splitext(name)[0]
        mvsnet_to_gipuma_cam(os.path.join(depth_folder, prefix + ".txt"), os.path.join(cam_folder, name + ".P"))
        shutil.copy(os.path.join(depth_folder, name), os.path.join(image_folder, name))
        sub = os.path.join(gipuma_point_folder, "2333__" + prefix)
        os.makedirs(sub, exist_ok=True)
        mvsnet_to_gipuma_dmb(os.path.join(depth_folder, prefix + "_prob_filtered.pfm"), os.path.join(sub, "disp.dmb"))
        fake_colmap_normal(os.path.join(sub, "disp.dmb"), os.path.join(sub, "normals.dmb"))
    return names


def fusibile_command(point_folder, fusibile_exe_path, disp_thresh, num_consistent):
    """depthfusion.py:192-211 as an argument list."""
    return [fusibile_exe_path, "-input_folder", point_folder + "/", "-p_folder", os.path.join(point_folder, "cams") + "/",
            "-images_folder", os.path.join(point_folder, "images") + "/", "--depth_min=0.001", "--depth_max=100000",
            "--normal_thresh=360", "--disp_thresh=" + str(disp_thresh), "--num_consistent=" + str(num_consistent)]


def depth_map_fusion(point_folder, fusibile_exe_path, disp_thresh, num_consistent):
    cmd = fusibile_command(point_folder, fusibile_exe_path, disp_thresh, num_consistent)
    print(" ".join(cmd))
    if not (fusibile_exe_path and os.path.isfile(fusibile_exe_path)):
        print("fusibile executable not found: skipping the fusion step (external tool, not part of this package)")
        return None
    return subprocess.run(cmd, check=False).returncode


def hip_fusion(dense_folder, point_folder, prob_threshold, reproj_threshold, depth_rel_threshold, num_consistent,
               dedupe=True, fusion_sources="all", eval_gt=None, eval_max_dist=20.0, eval_thresholds=(), normals=False,
               normal_angle_threshold=None, jump_threshold=0.05, write_normal_maps=False, mesh=False, mesh_clean=None,
               mesh_simplify_voxels=None, mesh_eval_spacing=None, mesh_smooth=None, mesh_recolour=None):
    """--fusion hip: mvsnet_amd.fusion over depths_mvsnet/ -> <point_folder>/consistencyCheck-<time>/final3d_model.ply
    (with normals: x y z nx ny nz red green blue; write_normal_maps: depths_mvsnet/<idx>_normal.pfm, camera frame).
    With eval_gt (a PLY), the fused cloud is evaluated against it on the device (mvsnet_amd.evaluate) and the metrics are
    written to metrics.json next to the PLY.  With mesh, mvsnet_amd.mesh writes mesh.ply beside it: TSDF fusion and surface
    nets of the same depth maps under the same consistency criteria, then the stages of mvsnet_amd.mesh.STAGES that are asked
    for, in that table's order: mesh_clean = dict(min_component_faces=, min_component_extent=, keep_largest=),
    mesh_simplify_voxels = S, mesh_smooth = dict(iterations=, lam=, mu=, boundary=, max_voxels=) and mesh_recolour =
    dict(min_cos=, angle_power=, occlusion_rel=), the last two as their modules' check_arguments give them.  With mesh, eval_gt and mesh_eval_spacing = s the mesh, as it is written, is evaluated against the same
    ground truth by its surface samples at spacing s (mvsnet_amd.mesh_sample) into mesh_metrics.json beside mesh.ply;
    metrics.json stays the cloud's."""
    import json
    import time
    from . import fusion
    indices, depths, probs, cams, images = fusion.load_dense_folder(dense_folder)
    sources = fusion.listed_sources(dense_folder, indices) if fusion_sources == "listed" else None
    plan = fusion.FusionPlan(depths, probs, cams, images, prob_threshold=prob_threshold, reproj_threshold=reproj_threshold,
                             depth_rel_threshold=depth_rel_threshold, num_consistent=num_consistent, sources=sources,
                             dedupe=dedupe, normals=normals, normal_angle_threshold=normal_angle_threshold,
                             jump_threshold=jump_threshold)
    plan.enqueue()
    res = plan.result(with_normals=plan.normals)
    xyz, rgb, nrm = res[0], res[1], (res[3] if plan.normals else None)
    if write_normal_maps:
        maps = fusion.estimate_normals(plan.depth, plan.prob, cams, prob_threshold=prob_threshold, jump_threshold=jump_threshold,
                                       frame="camera")
        for i, m in zip(indices, maps):
            write_pfm(os.path.join(dense_folder, "depths_mvsnet", "%d_normal.pfm" % i), m)
    out = os.path.join(point_folder, "consistencyCheck-" + time.strftime("%Y%m%d-%H%M%S"))
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "final3d_model.ply")
    fusion.write_ply(path, xyz, rgb, nrm)
    print("fused %d views into %d points: %s" % (len(indices), len(xyz), path))
    if eval_gt:
        from . import evaluate
        gt, _ = evaluate.read_ply_points(eval_gt)
        metrics = evaluate.evaluate_point_clouds(plan.xyz[:len(xyz)], gt, max_dist=eval_max_dist, thresholds=eval_thresholds)
        with open(os.path.join(out, "metrics.json"), "w") as f:
            f.write(json.dumps(metrics) + "\n")
        print("evaluated against %s: %s" % (eval_gt, json.dumps(metrics)))
    if mesh:
        from .mesh import mesh_dense_folder, stage_keywords
        options = dict(mesh_clean or {}, simplify_voxels=mesh_simplify_voxels)
        options.update(stage_keywords(dict(smooth=mesh_smooth, recolour=mesh_recolour)))
        if mesh_eval_spacing is not None:
            options.update(eval_gt=eval_gt, eval_spacing=mesh_eval_spacing, eval_max_dist=eval_max_dist, eval_thresholds=eval_thresholds)
        print("meshed: %s" % json.dumps(mesh_dense_folder(
            dense_folder, os.path.join(out, "mesh.ply"), fusion_sources=fusion_sources, prob_threshold=prob_threshold,
            reproj_threshold=reproj_threshold, depth_rel_threshold=depth_rel_threshold, num_consistent=num_consistent, **options)))
    return path


def _build_parser():
    """-> (the parser, [(stage, its actions)] for the --mesh_* flags of mvsnet_amd.mesh's stages added before --mesh_eval_spacing,
    the same for those after it): the stages by age, as in mvsnet_amd.mesh's own parser; a new one goes last."""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dense_folder", type=str, required=True)
    ap.add_argument("--fusibile_exe_path", type=str, default="")
    ap.add_argument("--prob_threshold", type=float, default=0.8)
    ap.add_argument("--disp_threshold", type=float, default=0.25, help="fusibile's disparity threshold (--fusion fusibile only)")
    ap.add_argument("--num_consistent", type=float, default=3)
    ap.add_argument("--fusion", choices=("fusibile", "hip"), default="fusibile",
                    help="fusibile: Gipuma hand-off + the external binary (default); hip: this project's GPU fusion")
    ap.add_argument("--reproj_threshold", type=float, default=1.0, help="--fusion hip: reprojection error limit in pixels")
    ap.add_argument("--depth_rel_threshold", type=float, default=0.01, help="--fusion hip: relative depth error limit")
    ap.add_argument("--no_dedupe", action="store_true", help="--fusion hip: every view independent (witnesses not consumed)")
    ap.add_argument("--fusion_sources", choices=("all", "listed"), default="all",
                    help="--fusion hip: every other view, or the neighbours of pair.txt / covisibility.json in the dense folder")
    ap.add_argument("--eval_gt", type=str, default=None,
                    help="--fusion hip: ground-truth PLY; the fused cloud is evaluated against it (metrics.json beside the PLY)")
    ap.add_argument("--eval_max_dist", type=float, default=20.0, help="--eval_gt: distance cap (outliers at or beyond it)")
    ap.add_argument("--eval_thresholds", type=str, default="", help="--eval_gt: comma-separated tau for precision / recall / F")
    ap.add_argument("--normals", action="store_true", help="--fusion hip: estimate normals, PLY vertices x y z nx ny nz r g b")
    ap.add_argument("--normal_angle_threshold", type=float, default=None,
                    help="--fusion hip: pairs whose normals differ by this many degrees or more are inconsistent (implies --normals)")
    ap.add_argument("--jump_threshold", type=float, default=None,
                    help="--fusion hip: relative depth jump beyond which a neighbour is not used for a normal (0.05)")
    ap.add_argument("--write_normal_maps", action="store_true",
                    help="--fusion hip: write depths_mvsnet/<idx>_normal.pfm (colour PFM, camera frame)")
    ap.add_argument("--mesh", action="store_true",
                    help="--fusion hip: also write mesh.ply beside final3d_model.ply (mvsnet_amd.mesh, default options)")
    from .mesh import FLAG_ORDER
    from .mesh_sample import add_options as add_sampling
    early = [(stage, stage.module.add_options(ap, "mesh_")) for stage in FLAG_ORDER[:2]]
    add_sampling(ap, "mesh_eval_")                                             # stands here since before the later stages came
    late = [(stage, stage.module.add_options(ap, "mesh_")) for stage in FLAG_ORDER[2:]]
    return ap, early, late


def build_parser():
    return _build_parser()[0]


def main(argv=None):
    from .mesh import stage_keywords
    ap, early, late = _build_parser()
    a = ap.parse_args(argv)
    mesh_stages = {}

    def need_mesh(actions):                                                    # a stage's flag away from its default asks for a mesh
        for action in actions:
            if getattr(a, action.dest) != action.default and not a.mesh:
                raise SystemExit("%s needs --mesh" % action.option_strings[0])

    def check(stage):
        try:
            mesh_stages[stage.name] = stage.module.check_arguments(a, "mesh_")
        except ValueError as e:
            raise SystemExit(str(e))

    # The checks go from the newest flag to the oldest, and say the same as ever when several things are wrong at once: the
    # stages after --mesh_eval_spacing ask for --mesh before they check their values, the older ones after.
    for stage, actions in reversed(late):
        need_mesh(actions)
        check(stage)
    if a.mesh_eval_spacing is not None:
        if not (a.mesh and a.eval_gt):
            raise SystemExit("--mesh_eval_spacing needs --mesh and --eval_gt")
        from .mesh_sample import check_spacing
        try:
            check_spacing(a.mesh_eval_spacing)
        except ValueError as e:
            raise SystemExit("--mesh_eval_spacing: %s" % e)
    for stage, actions in reversed(early):
        check(stage)
        need_mesh(actions)
    if a.fusion != "hip":
        for flag, given in (("--mesh", a.mesh), ("--normals", a.normals), ("--normal_angle_threshold", a.normal_angle_threshold is not None),
                            ("--jump_threshold", a.jump_threshold is not None), ("--write_normal_maps", a.write_normal_maps)):
            if given:
                raise SystemExit("%s needs --fusion hip" % flag)
    else:
        from .fusion import check_jump_threshold, normal_cos_threshold
        try:
            normal_cos_threshold(a.normal_angle_threshold)
            check_jump_threshold(0.05 if a.jump_threshold is None else a.jump_threshold)
        except ValueError as e:
            raise SystemExit(str(e))
    eval_thresholds = [float(v) for v in a.eval_thresholds.split(",") if v.strip()]
    if a.eval_gt:
        from .evaluate import check_thresholds
        if a.fusion != "hip":
            raise SystemExit("--eval_gt needs --fusion hip")
        try:
            check_thresholds(eval_thresholds, a.eval_max_dist)
        except ValueError as e:
            raise SystemExit("--eval_gt: %s" % e)
    if a.fusion == "hip":
        from ._lib import gpu_ready
        why = gpu_ready()
        if why is not None:
            raise SystemExit("--fusion hip needs a GPU and the HIP library: %s" % why)
    point_folder = os.path.join(a.dense_folder, "points_mvsnet")
    os.makedirs(point_folder, exist_ok=True)
    print("filter depth map with probability map")
    probability_filter(a.dense_folder, a.prob_threshold)
    if a.fusion == "hip":
        print("Run depth map fusion & filter on the GPU")
        return hip_fusion(a.dense_folder, point_folder, a.prob_threshold, a.reproj_threshold, a.depth_rel_threshold,
                          a.num_consistent, dedupe=not a.no_dedupe, fusion_sources=a.fusion_sources, eval_gt=a.eval_gt,
                          eval_max_dist=a.eval_max_dist, eval_thresholds=eval_thresholds, normals=a.normals,
                          normal_angle_threshold=a.normal_angle_threshold,
                          jump_threshold=0.05 if a.jump_threshold is None else a.jump_threshold,
                          write_normal_maps=a.write_normal_maps, mesh=a.mesh, mesh_eval_spacing=a.mesh_eval_spacing,
                          mesh_clean=stage_keywords(dict(clean=mesh_stages["clean"])), mesh_simplify_voxels=a.mesh_simplify_voxels,
                          mesh_smooth=mesh_stages["smooth"], mesh_recolour=mesh_stages["recolour"])
    print("Convert mvsnet output to gipuma input")
    mvsnet_to_gipuma(a.dense_folder, point_folder)
    print("Run depth map fusion & filter")
    depth_map_fusion(point_folder, a.fusibile_exe_path, a.disp_threshold, a.num_consistent)


if __name__ == "__main__":
    main()
