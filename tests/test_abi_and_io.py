"""CPU tests: the C-ABI library builds, loads and exports every symbol include/mvsnet_hip.h
declares (no compute calls without a GPU); PFM / camera formats are byte-compatible."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from oracle import mvsnet_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    text = open(os.path.join(ROOT, "include", "mvsnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mvs_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(lib_built):
    from mvsnet_amd import _lib
    syms = header_symbols()
    assert len(syms) >= 20
    assert sorted(_lib.SIGNATURES) == syms          # binding table and header agree
    lib = ctypes.CDLL(lib_built)
    for s in syms:
        assert hasattr(lib, s), s
    h = _lib.load()
    assert h.mvs_abi_version() == 1
    assert h.mvs_error_string(0) == b"success"
    assert b"bad argument" in h.mvs_error_string(-1)
    assert h.mvs_regnet_workspace_bytes(8, 8, 8, 32, 8) > 0
    assert h.mvs_set_conv_impl(7) == -1 and h.mvs_set_conv_impl(0) == 0
    # argument validation happens before any HIP call, so it is testable without a GPU
    assert h.mvs_softargmin_prob_f32(None, 8, 8, 8, 1.0, 1.0, 0, None, None, None) == -1
    assert h.mvs_regnet_us0_f32(None, 8, 8, 8, 32, 8, None, None, None, 1e-5, None, 0, None, None) == -1


def test_product_refuses_cpu_tensors(lib_built):
    import torch
    from mvsnet_amd import _lib
    with pytest.raises(_lib.MvsnetHipError):
        _lib.ptr(torch.zeros(4))


def test_pfm_roundtrip_and_bytes(tmp_path):
    from mvsnet_amd import preprocess as P
    img = np.array([[1, 2], [3, 4]], np.float32)
    exp = b"Pf\n2 2\n-1.000000\n" + np.array([3, 4, 1, 2], "<f4").tobytes()
    assert P.pfm_encode(img) == exp == O.pfm_bytes(img)
    rs = np.random.RandomState(0)
    big = rs.standard_normal((13, 7)).astype(np.float32)
    path = str(tmp_path / "x.pfm")
    P.write_pfm(path, big)
    assert open(path, "rb").read() == O.pfm_bytes(big)
    assert np.array_equal(P.load_pfm(path), big)
    assert np.array_equal(P.load_pfm(io.BytesIO(P.pfm_encode(big[:, :, None]))), big)
    col = rs.standard_normal((4, 5, 3)).astype(np.float32)
    assert np.array_equal(P.load_pfm(io.BytesIO(P.pfm_encode(col))), col)
    with pytest.raises(Exception):
        P.pfm_encode(big.astype(np.float64))
    with pytest.raises(Exception):
        P.load_pfm(io.BytesIO(b"P6\n1 1\n"))
    # big-endian files (positive scale) are read too
    be = b"Pf\n2 1\n1.000000\n" + np.array([5, 6], ">f4").tobytes()
    assert np.array_equal(P.load_pfm(io.BytesIO(be)), np.array([[5, 6]], np.float32))


def _cam_words(n_tail):
    ext = " ".join(str(float(v)) for v in range(16))
    intr = " ".join(str(float(v)) for v in range(100, 109))
    tail = ["425.0", "2.5", "192", "935.0"][:n_tail]
    return "extrinsic\n" + ext + "\n\nintrinsic\n" + intr + "\n\n" + " ".join(tail) + "\n"


def test_load_cam_word_count_variants(tmp_path):
    from mvsnet_amd import preprocess as P
    c29 = P.load_cam(io.StringIO(_cam_words(2)), interval_scale=1.06, max_d=128)
    assert np.array_equal(c29[0], np.arange(16.0).reshape(4, 4))
    assert np.array_equal(c29[1][:3, :3], np.arange(100.0, 109).reshape(3, 3))
    np.testing.assert_allclose(c29[1][3], [425, 2.65, 128, 425 + 2.65 * 128])
    with pytest.raises(ValueError):
        P.load_cam(io.StringIO(_cam_words(2)))
    c30 = P.load_cam(io.StringIO(_cam_words(3)), interval_scale=2)
    np.testing.assert_allclose(c30[1][3], [425, 5.0, 192, 425 + 5.0 * 192])
    c31 = P.load_cam(io.StringIO(_cam_words(4)))
    np.testing.assert_allclose(c31[1][3], [425, 2.5, 192, 935])
    path = str(tmp_path / "cam.txt")
    P.write_cam(path, c31)
    back = P.load_cam(path)
    assert np.array_equal(back, c31)
    assert open(path).read().startswith("extrinsic\n0.0 1.0 2.0 3.0 \n")


def test_png_quantisation():
    from mvsnet_amd import preprocess as P
    assert list(P.depth_to_uint16(np.array([-3.0, 12.7, 70000.0]))) == [0, 12, 65535]
    assert list(P.confidence_to_uint16(np.array([0.0, 0.5, 1.5]))) == [0, 32767, 65535]


def test_every_package_module_imports_without_a_gpu():
    """Import-time errors (syntax, missing names) in modules that only run on the GPU box must show up here."""
    import importlib
    import pkgutil
    import mvsnet_amd
    names = sorted(m.name for m in pkgutil.iter_modules(mvsnet_amd.__path__) if not m.name.startswith("lib"))   # not the .so
    assert {"inference", "train", "backward", "feature_net_train", "model", "test"} <= set(names)
    for name in names:
        importlib.import_module("mvsnet_amd." + name)
    for extra in ("bench", "__graft_entry__"):
        importlib.import_module(extra)


def test_ptr_refuses_tensors_of_another_device(monkeypatch):
    """One process drives one GPU: kernels launch on HIP's current device, so a tensor of any other device must be
    refused before its pointer reaches a launch (multi-GPU inference never bound its device)."""
    import torch
    from mvsnet_amd import _lib

    class FakeDev:
        index = 1

    class FakeTensor:
        is_cuda = True
        device = FakeDev()

        def is_contiguous(self):
            return True

        def data_ptr(self):
            return 0x1000
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    with pytest.raises(_lib.MvsnetHipError, match="current device"):
        _lib.ptr(FakeTensor())
    with pytest.raises(_lib.MvsnetHipError, match="current device"):
        _lib.ptr_array([None, FakeTensor()])
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 1)
    assert _lib.ptr(FakeTensor()).value == 0x1000


def test_bind_device_refuses_a_rank_without_a_gpu(monkeypatch):
    import torch
    from mvsnet_amd import shard
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 2)
    with pytest.raises(RuntimeError, match="only 2 GPU"):
        shard.bind_device(3)


def test_package_import_switches_off_the_miopen_solver_that_over_reads_its_filter():
    """mvsnet_amd/__init__.py: MIOpen's NHWC implicit-GEMM assembly kernel for the data gradient reads past the end of its
    filter tensor when the output-channel count is below its K tile (a GPU memory fault in narrow-tower training when the
    filter is the last block of an allocator segment, round 2); the package default disables that solver unless the user
    set the variable, and it must be in place before the first convolution."""
    import importlib
    import os
    import mvsnet_amd
    importlib.reload(mvsnet_amd)
    assert os.environ.get("MIOPEN_DEBUG_CONV_IMPLICIT_GEMM_ASM_BWD_GTC_XDLOPS_NHWC") in ("0", "1")
    saved = os.environ.pop("MIOPEN_DEBUG_CONV_IMPLICIT_GEMM_ASM_BWD_GTC_XDLOPS_NHWC")
    try:
        importlib.reload(mvsnet_amd)
        assert os.environ["MIOPEN_DEBUG_CONV_IMPLICIT_GEMM_ASM_BWD_GTC_XDLOPS_NHWC"] == "0"
        assert mvsnet_amd.ensure_miopen_workaround("test") is True
        os.environ[mvsnet_amd.MIOPEN_WORKAROUND] = "1"          # the user's explicit choice is kept, with a warning
        import pytest
        with pytest.warns(UserWarning, match="igemm_bwd_gtcx35_nhwc"):
            assert mvsnet_amd.ensure_miopen_workaround("test") is False
    finally:
        os.environ["MIOPEN_DEBUG_CONV_IMPLICIT_GEMM_ASM_BWD_GTC_XDLOPS_NHWC"] = saved


def _hazard_scanner():
    import importlib.util
    spec = importlib.util.spec_from_file_location("store_hazard_scan", os.path.join(ROOT, "tools", "store_hazard_scan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_no_wide_store_has_its_data_registers_overwritten_too_early(lib_built):
    """tools/store_hazard_scan.py over every gfx950 code object of the library.  Measured on MI355X (tools/store_hazard_probe.hip,
    profiles/r05_store_hazard_probe.txt): a 128-bit VMEM store whose data registers a VALU instruction overwrites fewer than
    2 wait states later (1 with a register in the soffset field) reaches memory corrupted in its first dword for ~2e-4 of the
    stores (lanes 12-15 of each row of 16) -- and the compiler inserts only 1 (0) wait state(s).  Round 5 lost the x component
    of float4 stores of the fused ConvGRU kernel that way; this test keeps every rebuild of the library honest."""
    import subprocess, sys
    if not _hazard_scanner().have_objdump():
        pytest.skip("llvm-objdump of ROCm not installed")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "store_hazard_scan.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "gru_fused.o" in r.stdout and " 0 with their data overwritten" in r.stdout


HAZARD_LISTING = """
0000000000001000 <kernel_a>:
\tv_mov_b32_e32 v9, 0                                     // 000000001000: 7E120280
0000000000001004 <L0>:
\t%(first)s
\tv_add_f32_e32 v20, v21, v22
\tglobal_store_dwordx4 v[0:1], v[4:7], off
\t%(after)s
\ts_cbranch_scc1 L0
\ts_endpgm
0000000000002000 <kernel_b>:
0000000000002000 <L0>:
\tv_mov_b32_e32 v4, 0
\ts_endpgm
"""


def test_store_hazard_scanner_follows_branches():
    """The scan walks the control flow after a wide store (VERDICT r5 item 13 / ADVICE r5): a data register overwritten by the
    first vector instruction of the NEXT loop iteration (back-edge), on the fall-through of a conditional branch, through an
    s_nop that is too short, by v_swap's second operand or in an AGPR is found; enough wait states, or a same-named label of
    another function, are not."""
    hz = _hazard_scanner()
    scan = lambda **kw: hz.scan_text(HAZARD_LISTING % kw)
    n, f = scan(first="v_mul_f32_e32 v5, v1, v2", after="")
    assert n == 1 and len(f) == 1 and "v_mul_f32_e32 v5" in f[0][2] and f[0][3] == 1       # back-edge: the branch is the one wait state
    n, f = scan(first="v_mul_f32_e32 v5, v1, v2", after="s_add_u32 s0, s0, 1")
    assert n == 1 and not f                                                                # scalar instruction + branch = two wait states
    n, f = scan(first="v_mul_f32_e32 v8, v1, v2", after="")
    assert not f                                                                           # other registers (and kernel_b's L0 is not ours)
    n, f = scan(first="v_swap_b32 v30, v7", after="")
    assert len(f) == 1
    n, f = scan(first="s_mov_b32 s1, 0", after="v_mfma_f32_16x16x4_f32 v[4:7], v8, v9, v[4:7]")
    assert len(f) == 1 and f[0][3] == 0                                                    # straight line, no wait state at all
    n, f = scan(first="s_mov_b32 s1, 0", after="s_nop 0\n\tv_mfma_f32_16x16x4_f32 v[4:7], v8, v9, v[4:7]")
    assert len(f) == 1 and f[0][3] == 1                                                    # the compiler's single wait state is not enough
    n, f = scan(first="s_mov_b32 s1, 0", after="s_nop 1\n\tv_mfma_f32_16x16x4_f32 v[4:7], v8, v9, v[4:7]")
    assert not f
    lst = HAZARD_LISTING.replace("global_store_dwordx4 v[0:1], v[4:7], off", "buffer_store_dwordx4 a[4:7], v0, s[0:3], 0 offen")
    n, f = hz.scan_text(lst % dict(first="v_accvgpr_write_b32 a6, v1", after=""))
    assert n == 1 and len(f) == 1
    lst = HAZARD_LISTING.replace("global_store_dwordx4 v[0:1], v[4:7], off", "buffer_store_dwordx4 v[4:7], v0, s[0:3], s9 offen")
    n, f = hz.scan_text(lst % dict(first="v_mul_f32_e32 v5, v1, v2", after=""))
    assert n == 1 and not f                                                                # register soffset: one wait state is enough


def test_test_hooks_and_fused_route_without_a_gpu(lib_built):
    """mvs_set_test_hook replaces the eight environment switches of round 5: ids, ranges and defaults;
    mvs_gru_fused_route is the routing predicate mvs_gru_wta*_f32 evaluate before anything is enqueued (a view block
    of 2 GiB or more must take the wavefront route, not fail inside the sweep)."""
    from mvsnet_amd import _lib
    h = _lib.load()
    text = open(os.path.join(ROOT, "include", "mvsnet_hip.h")).read()
    ids = dict(re.findall(r"#define MVS_HOOK_([A-Z0-9_]+)\s+(\d+)", text))
    count = int(ids.pop("COUNT"))
    assert {k.lower(): int(v) for k, v in ids.items()} == _lib.HOOKS and count == len(_lib.HOOKS)
    for name, hid in _lib.HOOKS.items():
        assert h.mvs_get_test_hook(hid) == _lib.HOOK_DEFAULTS[name], name
    assert h.mvs_set_test_hook(count, 0) == -1 and h.mvs_get_test_hook(-1) == -1 and h.mvs_get_test_hook(count) == -1
    for name, bad in (("cv_tile_rows_log2", 4), ("cv_tile_rows_log2", -2), ("conv_no_span", 2), ("s2_planes", -1),
                      ("gru_one_stream", 7), ("gru_producer_threads", 0), ("gru_producer_threads", 100), ("gru_producer_threads", 512)):
        assert h.mvs_set_test_hook(_lib.HOOKS[name], bad) == -1, (name, bad)
        assert h.mvs_get_test_hook(_lib.HOOKS[name]) == _lib.HOOK_DEFAULTS[name]
    with _lib.test_hooks(s2_planes=3, gru_producer_threads=192):
        assert h.mvs_get_test_hook(_lib.HOOKS["s2_planes"]) == 3 and h.mvs_get_test_hook(_lib.HOOKS["gru_producer_threads"]) == 192
    assert h.mvs_get_test_hook(_lib.HOOKS["s2_planes"]) == 0
    # no getenv left in the product sources
    import glob
    for f in glob.glob(os.path.join(ROOT, "mvsnet_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "mvsnet_amd", "csrc", "*.h")):
        src = re.sub(r"//.*", "", open(f).read())
        assert "getenv" not in src, f
    # routing of the recurrent sweep: c3 (400 x 300) is fused, 576 x 384 is not, other filter counts are not
    blk = lambda H, W: h.mvs_gru_workspace_bytes(H, W, 32, 16, 4, 2)
    assert blk(300, 400) < 2 ** 31 and h.mvs_gru_fused_route(32, 16, 4, 2, blk(300, 400)) == 1
    assert blk(384, 576) >= 2 ** 31 and h.mvs_gru_fused_route(32, 16, 4, 2, blk(384, 576)) == 0
    assert h.mvs_gru_fused_route(32, 32, 8, 4, blk(300, 400)) == 0 and h.mvs_gru_fused_route(16, 16, 4, 2, blk(300, 400)) == 0


def test_gru_workspace_layout_is_pinned(lib_built):
    """mvs_gru_workspace_bytes (H, W, C, f1, f2, f3) -> bytes per view block, as commit 5de61d1 (the last one with the sweep
    inside csrc/gru.hip) returned them: mvsnet_amd/model.py allocates by this number and the fused kernels address the block
    with 32-bit offsets from its base, so a change of the carving is a change of the ABI."""
    from mvsnet_amd import _lib
    h = _lib.load()
    pinned = {(300, 400, 32, 16, 4, 2): 1222399744,      # 5de61d1
              (384, 576, 32, 16, 4, 2): 2252857600,      # 5de61d1
              (5, 11, 32, 16, 4, 2): 885504,             # 5de61d1
              (27, 41, 16, 8, 2, 1): 5850368,            # 5de61d1
              (27, 41, 64, 32, 8, 4): 23356928,          # 5de61d1
              (27, 41, 16, 12, 6, 3): 8543488}           # 5de61d1
    for shape, want in pinned.items():
        assert h.mvs_gru_workspace_bytes(*shape) == want, shape
