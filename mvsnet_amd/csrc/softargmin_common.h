// The two formulas the soft-argmin forward (softargmin.hip) and backward (backward.hip) must agree on bit for bit: the depth
// of plane d and the four probability buckets around a regressed depth.  The backward treats the bucket indices as constants
// of the forward, so both sides have to choose the same ones.
#pragma once

__device__ __forceinline__ float depth_at(int d, int D, float start, float interval, int inverse) {
    float end = start + ((float)D - 1.0f) * interval;                    // model.py:378-379
    float denom = (float)(D > 1 ? D - 1 : 1);
    if (inverse) {                                                        // :481-485
        float a = 1.0f / start, b = 1.0f / end;
        return 1.0f / (a + (float)d * ((b - a) / denom));
    }
    return start + (float)d * ((end - start) / denom);                    // :487-488
}

// Planes of the probability map P[l0] + P[r0] + P[l1] + P[r1] (model.py:83-140): floor / ceil of the depth's plane index and
// their outer neighbours, clamped to the volume.  Inverse depth counts the planes from the far end.
__device__ __forceinline__ void prob_buckets(float depth, int D, float start, float interval, int inverse,
                                             int& l0, int& r0, int& l1, int& r1) {
    int l, r;
    if (inverse) {
        float end = start + ((float)D - 1.0f) * interval;
        float inv_s = 1.0f / start, inv_e = 1.0f / end;
        float inv_int = (inv_s - inv_e) / ((float)D - 1.0f);
        float idx = (1.0f / depth - inv_e) / inv_int;
        l = D - (int)ceilf(idx) - 1;
        r = D - (int)floorf(idx) - 1;
    } else {
        float idx = (depth - start) / interval;
        l = (int)floorf(idx);
        r = (int)ceilf(idx);
    }
    l0 = min(max(l, 0), D - 1);
    r0 = min(max(r, 0), D - 1);
    l1 = min(max(l0 - 1, 0), D - 1);
    r1 = min(max(r0 + 1, 0), D - 1);
}
