"""Camera families for the cost-volume backward tests: `synthetic.make_cams` with the SOURCE views changed.

A plain helper module (no fixtures, no GPU): tests/test_cost_backward_window_host.py holds a numpy restatement of the gather
kernel's candidate window against the true contributors under every family, tests/test_gpu_cost_backward_cameras.py runs
both backward kernels under them.

`make_cams` alone gives one benign geometry: every view shares one K and rotates about the y axis round the pivot (0, 0, 650 mm)
by a few degrees, without roll or zoom, so the plane homographies are close to a shift along x.  The families keep the
reference view and the pivot -- the pivot stays on every source camera's optical axis unless the family moves it -- and change:

  roll30 roll90 roll180      the source cameras turn about their own optical axis (the homography turns the image)
  zoom0.5 zoom0.25 zoom2 zoom4   the source focal length is scaled (minification / magnification of the window by 1 / zoom)
  zoom0.125 zoom0.1          minification beyond 8: the gather window asks for more than 8 pixels (9.4 at 0.125)
  wide25 wide45              y-rotation about the pivot by -a, +a, -a, ... degrees instead of make_cams' few
  tilt20                     x-rotation about the pivot by -20, +20, ... degrees
  random0 .. random3         seeded: rotations about all three axes (y and x within 15 degrees about the pivot, roll anywhere),
                             the pivot moved off the axis by up to 40 mm in x and y and 60 mm in depth, focal length x a
                             log-uniform factor in [0.3, 3], principal point moved by up to a tenth of the image

RANDOM_SEEDS are the first seeds at which every source view keeps at least 100 in-image (source pixel, reference pixel) pairs at
3 views, 24 x 32 pixels, 8 planes (the host test asserts it for every family); seeds whose views leave the image are not listed.
60 degrees of y-rotation leaves the image as well and is no family.
"""
import math

import numpy as np

from mvsnet_amd import synthetic as S
from oracle import mvsnet_oracle as O

RANDOM_SEEDS = (0, 1, 2, 3)
NAMED = ("roll30", "roll90", "roll180", "zoom0.5", "zoom0.25", "zoom2", "zoom4", "wide25", "wide45", "tilt20")
RANDOM = tuple("random%d" % k for k in range(len(RANDOM_SEEDS)))
EXTREME = ("zoom0.125", "zoom0.1")                # more than 8 pixels of window
FAMILIES = NAMED + RANDOM + EXTREME

PIVOT = np.array([0.0, 0.0, S.PIVOT_DEPTH])


def rot(axis, degrees):
    a = math.radians(degrees)
    c, s = math.cos(a), math.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]),
            "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])}[axis]


def _set_pose(cam, R, pivot_in_camera=PIVOT):
    """World -> camera rotation R with the pivot at `pivot_in_camera` of the camera's frame."""
    cam[0, :3, :3] = R
    cam[0, :3, 3] = pivot_in_camera - R @ PIVOT


def _randomise(cam, seed, v, height, width):
    rs = np.random.RandomState(7919 * seed + v)
    ay, ax, az = rs.uniform(-15, 15), rs.uniform(-15, 15), rs.uniform(-180, 180)
    shift = np.array([rs.uniform(-40, 40), rs.uniform(-40, 40), rs.uniform(-60, 60)])
    _set_pose(cam, rot("z", az) @ (rot("y", ay) @ rot("x", ax)).T, PIVOT + shift)
    zoom = math.exp(rs.uniform(math.log(0.3), math.log(3.0)))
    cam[1, 0, 0] *= zoom; cam[1, 1, 1] *= zoom
    cam[1, 0, 2] += rs.uniform(-0.1, 0.1) * width; cam[1, 1, 2] += rs.uniform(-0.1, 0.1) * height


def make_family_cams(name, view_num, height, width, depth_num, seed=None):
    """cams (N, 2, 4, 4) float32 in make_cams' layout; view 0 is make_cams' reference view.  `seed`: for the name "random", any
    seed (the families random0 .. carry RANDOM_SEEDS)."""
    cams = S.make_cams(view_num, height, width, depth_num).astype(np.float64)
    for v in range(1, view_num):
        cam, sign = cams[v], (-1.0 if v % 2 else 1.0)
        if name.startswith("roll"):
            Rz = rot("z", sign * float(name[4:]))
            cam[0, :3, :3] = Rz @ cam[0, :3, :3]
            cam[0, :3, 3] = Rz @ cam[0, :3, 3]
        elif name.startswith("zoom"):
            cam[1, 0, 0] *= float(name[4:]); cam[1, 1, 1] *= float(name[4:])
        elif name.startswith("wide"):
            _set_pose(cam, rot("y", sign * float(name[4:])).T)
        elif name.startswith("tilt"):
            _set_pose(cam, rot("x", sign * float(name[4:])).T)
        elif name.startswith("random"):
            _randomise(cam, RANDOM_SEEDS[int(name[6:])] if seed is None else seed, v, height, width)
        else:
            raise KeyError(name)
    return cams.astype(np.float32)


def family_transforms(name, view_num, height, width, depth_num, seed=None):
    """-> t8 (N - 1, D, 8) float32: the eight coefficients per (source view, plane) the kernels take, formed as
    tests/test_gpu_backward.py's _toy_problem forms them."""
    cams = make_family_cams(name, view_num, height, width, depth_num, seed)
    start, interval = float(cams[0, 1, 3, 0]), float(cams[0, 1, 3, 1])
    Hs = np.stack([O.get_homographies(cams[0], cams[v], depth_num, start, interval, np.float32) for v in range(1, view_num)])
    return O.homography_to_transform8(Hs, np.float32)
