"""The mesh stages' command lines and error texts, held to what they were before the stages got one shared module
(mvsnet_amd.mesh_common) and one table (mvsnet_amd.mesh.STAGES).

tests/golden/mesh_stage_messages.json was recorded on the CPU from the commit named in its "recorded_on", the last one in
which every stage still carried its own copy of the plumbing.  It is a record, not an expectation that follows the code: when
an entry differs, the code is wrong.  Three kinds of entry:
  * "parsers": per command line, the ordered actions of its parser (``actions``);
  * "command_lines": argv that a command line refuses, with the payload of its SystemExit; what argparse itself refuses is
    recorded as the exit code 2 alone, the wording being argparse's.  "{TMP}" stands for a temporary directory, in which
    out.ply exists;
  * "calls": library calls that raise, with the exception's type and text.  Arguments are JSON, {"$": name} being NAMED[name].
    They run with no GPU visible (torch.cuda.is_available is patched), so a valid call ends in MvsnetHipError with the stage's
    own name in it, and nothing here touches a device.
"""
import contextlib
import importlib
import io
import json
import os

import numpy as np
import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_stage_messages.json")
COMMAND_LINES = ("mesh", "mesh_clean", "mesh_smooth", "mesh_simplify", "mesh_colour", "mesh_sample", "depthfusion")


class Shape:
    """Stands for an array too large to allocate: the shape checks read nothing else."""

    def __init__(self, *shape):
        self.shape = shape


V, F = np.ones((4, 3), np.float32), np.zeros((1, 3), np.int32)
NAMED = {
    "nan": float("nan"), "inf": float("inf"), "-inf": float("-inf"),
    "V": V, "F": F, "C": np.zeros((4, 3), np.uint8),
    "V_xy": V[:, :2], "F_2": F[:, :2], "F_flat": F[0], "C_3": np.zeros((3, 3), np.uint8),
    "V_nan": np.full((2, 3), np.nan, np.float32), "V_wide": np.array([[0, 0, 0], [3e6, 1, 1]], np.float32),
    "M_2^31": Shape(2 ** 31, 3), "F_2^31": Shape(2 ** 31, 3), "F_edges": Shape((2 ** 31 - 1) // 6 + 1, 3),
    "F_corners": Shape((2 ** 31 - 1) // 3 + 1, 3), "F_2^26+1": Shape(2 ** 26 + 1, 3),
    "Z": np.zeros((2, 4, 4), np.float32), "Z_cams": np.zeros((2, 2, 4, 4)),
    "cams": np.tile(np.eye(4), (3, 2, 1, 1)), "cams_2": np.tile(np.eye(4), (2, 2, 1, 1)), "cams_1x4x4": np.tile(np.eye(4), (3, 1, 1, 1)),
    "images": [np.zeros((6, 8, 3), np.uint8)] * 3, "images_2ch": [np.zeros((6, 8, 2), np.uint8)] * 3,
    "images_f32": [np.zeros((6, 8, 3), np.float32)] * 3,
}


def decode(x):
    if isinstance(x, dict) and set(x) == {"$"}:
        return NAMED[x["$"]]
    if isinstance(x, dict):
        return {k: decode(v) for k, v in x.items()}
    return [decode(v) for v in x] if isinstance(x, list) else x


def plain(x):
    """A parser's default, choices or exit payload as JSON holds it."""
    return list(x) if isinstance(x, tuple) else x


def actions(parser):
    """[[option strings, dest, action class, type name, default, choices, required, help]] in the order of --help."""
    return [[list(a.option_strings), a.dest, type(a).__name__, None if a.type is None else a.type.__name__, plain(a.default),
             None if a.choices is None else list(a.choices), bool(a.required), a.help] for a in parser._actions]


def refusal(module, argv, tmp):
    """What ``module.main(argv)`` raises: 2 for argparse's own exit, else the payload with the temporary directory as {TMP}."""
    argv = [a.replace("{TMP}", tmp) for a in argv]
    with contextlib.redirect_stderr(io.StringIO()), contextlib.redirect_stdout(io.StringIO()):
        try:
            importlib.import_module("mvsnet_amd." + module).main(argv)
        except SystemExit as e:
            return e.code if isinstance(e.code, int) else str(e.code).replace(tmp, "{TMP}")
    return "returned"


def extract(**stages):
    """TsdfVolume.extract on a volume that has no tensors: bad stage options must raise before any of them is touched."""
    from mvsnet_amd.mesh import TsdfVolume
    vol = object.__new__(TsdfVolume)
    vol.origin, vol.voxel, vol.dims = np.zeros(3, np.float32), 0.5, (4, 4, 4)
    return vol.extract(**stages)


def raised(call, args, kwargs):
    """[type name, text] of what the call raises."""
    if call == "extract":
        fn = extract
    else:
        module, name = call.split(".")
        fn = getattr(importlib.import_module("mvsnet_amd." + module), name)
    try:
        fn(*decode(args), **decode(kwargs))
    except Exception as e:
        return [type(e).__name__, str(e)]
    return ["returned", ""]


with open(FIXTURE) as _f:
    RECORD = json.load(_f)


@pytest.mark.parametrize("module", COMMAND_LINES)
def test_parsers_have_the_recorded_actions(module):
    got = actions(importlib.import_module("mvsnet_amd." + module).build_parser())
    assert len(got) == len(RECORD["parsers"][module])
    for g, want in zip(got, RECORD["parsers"][module]):
        assert g == want


@pytest.mark.parametrize("module", COMMAND_LINES)
def test_refused_command_lines_say_what_they_said(module, tmp_path):
    (tmp_path / "out.ply").write_bytes(b"")
    cases = [c for c in RECORD["command_lines"] if c["module"] == module]
    assert cases
    for c in cases:
        assert refusal(module, c["argv"], str(tmp_path)) == c["exit"], c["argv"]
    assert [p.name for p in tmp_path.iterdir()] == ["out.ply"] and not os.path.exists("none")


CALLS = sorted({c["call"] for c in RECORD["calls"]})


@pytest.mark.parametrize("call", CALLS)
def test_refused_library_calls_say_what_they_said(call, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for c in RECORD["calls"]:
        if c["call"] == call:
            assert raised(call, c["args"], c["kwargs"]) == c["raises"], (c["args"], c["kwargs"])


def test_the_record_covers_every_stage_and_names_its_commit():
    assert len(RECORD["recorded_on"]) == 40 and set(RECORD["parsers"]) == set(COMMAND_LINES)
    assert set(CALLS) == {"mesh_clean.clean_mesh", "mesh_clean.mesh_components", "mesh_smooth.smooth_mesh", "mesh_simplify.simplify_mesh",
                          "mesh_colour.colour_mesh", "mesh_colour.vertex_normals", "mesh_sample.sample_mesh", "mesh.mesh_depth_maps",
                          "extract"}
    no_gpu = [c["raises"][1].split(" runs on the GPU")[0] for c in RECORD["calls"] if c["raises"][0] == "MvsnetHipError"]
    assert sorted(set(no_gpu)) == ["mesh cleaning", "mesh colouring", "mesh sampling", "mesh simplification", "mesh smoothing"]
