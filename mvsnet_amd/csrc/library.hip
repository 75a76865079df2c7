// Library bookkeeping: ABI version, error strings, the regulariser's implementation selector, the test / measurement hooks
// and the enable / read-out entry points of the three live profilers.  No kernels and no launches here.
#include "profile.h"

extern "C" int mvs_abi_version(void) { return MVS_ABI_VERSION; }

extern "C" const char* mvs_error_string(int code) {
    if (code == 0) return "success";
    if (code == MVS_E_BADARG) return "mvsnet_hip: bad argument (null pointer or non-positive size)";
    if (code == MVS_E_SHAPE) return "mvsnet_hip: shape not supported by this kernel";
    if (code == MVS_E_WORKSPACE) return "mvsnet_hip: workspace too small";
    if (code == MVS_E_NO_SLOT) return "mvsnet_hip: all 16 stream sets of mvs_gru_prepare are in use (mvs_gru_release frees one); the sweep still runs, on the caller's stream alone";
    if (code == MVS_E_NOT_PREPARED) return "mvsnet_hip: no side streams for this caller stream (call mvs_gru_prepare outside hipGraph capture first)";
    if (code > 0) return hipGetErrorString((hipError_t)code);
    return "mvsnet_hip: unknown error";
}

static int g_conv_impl = MVS_CONV_IMPL_AUTO;
extern "C" int mvs_set_conv_impl(int impl) {
    if (impl < MVS_CONV_IMPL_AUTO || impl > MVS_CONV_IMPL_BF16X3) return MVS_E_BADARG;
    g_conv_impl = impl;
    return 0;
}
extern "C" int mvs_get_conv_impl(void) { return g_conv_impl; }

// test / measurement hooks (include/mvsnet_hip.h): the only switches of the library; nothing is read from the environment
#ifndef MVS_PAIR_DIRECT_DEFAULT      // A/B builds: -DMVS_PAIR_DIRECT_DEFAULT=1 is this library with the direct pair kernel as its default
#define MVS_PAIR_DIRECT_DEFAULT 0
#endif
#ifndef MVS_PAIR_WAVES4_DEFAULT      // A/B builds: -DMVS_PAIR_WAVES4_DEFAULT=1 is this library with the four-wave Winograd pair kernel as its default
#define MVS_PAIR_WAVES4_DEFAULT 0
#endif
std::atomic<int> mvs_hooks[MVS_HOOK_COUNT] = {{-1}, {0}, {0}, {0}, {0}, {128}, {1}, {0}, {0}, {0}, {0}, {0}, {0}, {0}, {0}, {0}, {0}, {MVS_PAIR_DIRECT_DEFAULT},
                                              {MVS_PAIR_WAVES4_DEFAULT}};
extern "C" int mvs_set_test_hook(int id, int value) {
    bool ok = false;
    switch (id) {
        case MVS_HOOK_CV_TILE_ROWS_LOG2: ok = value >= -1 && value <= 3; break;
        case MVS_HOOK_CONV_NO_SPAN: case MVS_HOOK_CONV_NO_FUSE2: case MVS_HOOK_GRU_ONE_STREAM: case MVS_HOOK_UNET_PERSISTENT:
        case MVS_HOOK_REGNET_SIDE_BRANCH: case MVS_HOOK_PAIR_DIRECT: case MVS_HOOK_PAIR_WAVES4:
            ok = value == 0 || value == 1; break;
        case MVS_HOOK_CONV_FULL_SWEEPS: ok = value >= 0 && value < 16 && (value & 3) < 3 && (value >> 2) < 3; break;
        case MVS_HOOK_UNET_GRID: ok = value >= 0 && value <= 65536; break;
        case MVS_HOOK_FUSE2_PLANES: case MVS_HOOK_PAIR_PLANES: ok = value >= 0 && value <= 65536 && (value & 1) == 0; break;
        case MVS_HOOK_S2_PLANES: case MVS_HOOK_OUT_PLANES: case MVS_HOOK_S1_PLANES: ok = value >= 0 && value <= 65536; break;
        case MVS_HOOK_SPAN_FORCE: ok = value == 0 || ((value >> 8) >= 1 && (value >> 8) <= 8 && (value & 255) >= (value >> 8) && (value & 255) <= 16); break;
        case MVS_HOOK_BN_SLOTS: case MVS_HOOK_PAIR_SLOTS: ok = value >= 0 && value <= 8; break;      // 8 = MVS_BN_SLOTS_MAX (regnet.hip asserts it)
        case MVS_HOOK_GRU_PRODUCER_THREADS: ok = value == 64 || value == 128 || value == 192 || value == 256; break;
        default: break;
    }
    if (!ok) return MVS_E_BADARG;
    mvs_hooks[id].store(value, std::memory_order_relaxed);
    return 0;
}
extern "C" int mvs_get_test_hook(int id) {
    if (id < 0 || id >= MVS_HOOK_COUNT) return MVS_E_BADARG;
    return mvs_hooks[id].load(std::memory_order_relaxed);
}

// ---- live profilers (profile.h): what bench.py's roofline object and roofline_kernels rows read ----------------------
// the dominant kernel: when enabled, every RegNetUS0 run brackets its first launch -- the fused 3dconv0_1 + 3dconv1_0 pass,
// ~45 % of a depth map -- with a pair of HIP events on the caller's stream
EventSlots<64, 2> mvs_prof_dominant;
EventSlots<32, 22> mvs_prof_layers;
EventSlots<32, 4> mvs_prof_stages;      // the split of the TIMED path, mvs_depth_from_features_f32

extern "C" int mvs_profile_dominant(int enable) { mvs_prof_dominant.enable(enable != 0); return 0; }
extern "C" int mvs_profile_dominant_ms(double* avg_ms, int* count) {
    MVS_CHECK_ARG(avg_ms && count);
    return mvs_prof_dominant.read(avg_ms, 1, 2, count);
}
extern "C" int mvs_profile_layers(int enable) { mvs_prof_layers.enable(enable != 0); return 0; }
extern "C" int mvs_profile_layers_ms(double* avg_ms11, int* count) {
    MVS_CHECK_ARG(avg_ms11 && count);
    return mvs_prof_layers.read(avg_ms11, 11, 2, count);
}
extern "C" int mvs_profile_stages(int enable) { mvs_prof_stages.enable(enable != 0); return 0; }
extern "C" int mvs_profile_stages_ms(double* avg_ms3, int* count) {
    MVS_CHECK_ARG(avg_ms3 && count);
    return mvs_prof_stages.read(avg_ms3, 3, 1, count);
}
