// splatco_amd/csrc/tsdf_node.h -- what the dense (tsdf.hip) and the block-sparse (tsdf_sparse.hip) TSDF families share on the
// device: the per-node update of one view (steps 1 to 5 of include/splatco_tsdf.h) and the lattice tables of the marching
// tetrahedra.  Both integration kernels call ts_node_update, so a node of a sparse block gets literally the code, and with it
// the bits, of the same node of a dense volume.  Everything between the float32 inputs and the float32 outputs is binary64 in
// the written order; the Makefile's -ffp-contract=off keeps it uncontracted.
#pragma once
#include "common.h"
#include "../../include/splatco_tsdf.h"

namespace scr {

__device__ __forceinline__ bool ts_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }     // false for NaN

// One view V applied to the node (ci, cj, ck) of the lattice g (g.lox, g.loy, g.loz, g.h, g.trunc, g.max_weight, binary64):
// s, w and (COLOR) c0..c2 are the node's stored float32 values, updated in place or left alone.  M = V.w2c and HW = V.H V.W
// are the caller's, taken once per view and not once per node.
template <bool COLOR, class Lattice>
__device__ __forceinline__ void ts_node_update(const Lattice& g, const scr_tsdf_view& V, const double* M, size_t HW, int ci, int cj, int ck,
                                               float& s, float& w, float& c0, float& c1, float& c2) {
    const double x = g.lox + g.h * (double)ci, y = g.loy + g.h * (double)cj, z = g.loz + g.h * (double)ck;
    const double xc = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
    const double yc = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
    const double zc = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
    if (!(zc > V.near)) return;
    const double u = V.fx * xc / zc + V.cx, v = V.fy * yc / zc + V.cy;
    const double fu = floor(u), fv = floor(v);
    if (!(fu >= 0.0 && fu < (double)V.W && fv >= 0.0 && fv < (double)V.H)) return;
    const size_t pix = (size_t)(int)fv * V.W + (size_t)(int)fu;
    const float D = V.depth[pix], A = V.alpha[pix];
    bool ok = ts_finite(D) && ts_finite(A) && A >= V.min_alpha && D > 0.0f;
    if (V.mask_kind == 1) ok = ok && ((const float*)V.mask)[pix] > 0.0f;
    if (V.mask_kind == 2) ok = ok && ((const uint8_t*)V.mask)[pix] != 0;
    if (!ok) return;
    const float zf = D / A;                                 // ONE binary32 division
    const double sdf = (double)zf - zc;
    if (sdf < -g.trunc) return;
    const double d = fmin(1.0, sdf / g.trunc);
    const double Wt = (double)w, den = Wt + 1.0;
    s = (float)(((double)s * Wt + d) / den);
    if (COLOR && V.image) {
        const float q0 = V.image[pix], q1 = V.image[HW + pix], q2 = V.image[2 * HW + pix];
        if (ts_finite(q0) && ts_finite(q1) && ts_finite(q2)) {
            c0 = (float)(((double)c0 * Wt + (double)q0) / den);
            c1 = (float)(((double)c1 * Wt + (double)q1) / den);
            c2 = (float)(((double)c2 * Wt + (double)q2) / den);
        }
    }
    w = (float)fmin(den, g.max_weight);
}

// ------------------------------------------------------------------ extraction: lattice tables
// a node offset inside a cube is a 3-bit code, bit 0 = +x, bit 1 = +y, bit 2 = +z
__device__ __forceinline__ int ts_dir_code(int dir) { return ((0x59 >> dir) & 1) | (((0x6A >> dir) & 1) << 1) | (((0x74 >> dir) & 1) << 2); }
// the lattice direction of an offset code 1..7: (1,0,0) (0,1,0) (1,1,0) (0,0,1) (1,0,1) (0,1,1) (1,1,1) -> 0 1 3 2 4 5 6
__device__ __forceinline__ int ts_code_dir(int code) { return (int)((0xD62640u >> (3 * code)) & 7u); }
// local node x = 0..3 of Kuhn tetrahedron q: corner, + e_pi1, + e_pi2, corner + (1, 1, 1); pi1 = q / 2, pi2 from a packed table
__device__ __forceinline__ int ts_tet_code(int q, int x) {
    const int a1 = q >> 1, a2 = (0x489 >> (2 * q)) & 3;
    return x == 0 ? 0 : x == 1 ? (1 << a1) : x == 2 ? ((1 << a1) | (1 << a2)) : 7;
}
constexpr uint32_t TS_FLIP_EVEN = 0x4D24;               // inside masks whose triangles swap their last two vertices (even pi)
constexpr uint32_t TS_ODD_PERM = 0x26;                  // q = 1, 2, 5: xzy, yxz, zyx

// the three edges of triangle `tri` (0 / 1) of tetrahedron q with inside mask m (1 .. 14), as pairs of local nodes, wound
// counter-clockwise seen from the outside
__device__ __forceinline__ void ts_triangle_edges(uint32_t m, int q, int tri, int (&ex)[3], int (&ey)[3]) {
    const uint32_t out = ~m & 15u;
    const int cnt = __builtin_popcount(m);
    if (cnt == 2) {
        const int a = __builtin_ctz(m), b = 31 - __builtin_clz(m), cc = __builtin_ctz(out), d = 31 - __builtin_clz(out);
        ex[0] = a; ey[0] = cc;
        if (tri == 0) { ex[1] = a; ey[1] = d; ex[2] = b; ey[2] = d; }
        else          { ex[1] = b; ey[1] = d; ex[2] = b; ey[2] = cc; }
    } else {
        const uint32_t one = cnt == 1 ? m : out;        // the single node, and the three others in ascending order
        uint32_t rest = ~one & 15u;
        const int a = __builtin_ctz(one);
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            ex[e] = a; ey[e] = __builtin_ctz(rest);
            rest &= rest - 1;
        }
    }
    if ((((TS_FLIP_EVEN >> m) ^ (TS_ODD_PERM >> q)) & 1u) != 0) {
        int t = ex[1]; ex[1] = ex[2]; ex[2] = t;
        t = ey[1]; ey[1] = ey[2]; ey[2] = t;
    }
}

}  // namespace scr
