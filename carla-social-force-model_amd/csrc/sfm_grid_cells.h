// sfm_grid_cells.h -- what the two grid kernels share: the rotation into the heading frame, the window with its cell rule, and the
// ordered accumulation of a list of sources into the cells a lane owns (sfm_batch_grid.hip grids around pedestrian rows,
// sfm_batch_vehicle_grid.hip around vehicles; the rules are specified in include/sfm_hip.h).  Each kernel keeps its front half --
// staging, what is gridded, the zero fills, its barriers -- its lists and its stores, and says what an item is.  Both keep their LDS,
// scratch and occupancy figures with the pieces here (csrc/resource_usage.txt).
#pragma once
#include "sfm_device.h"

#pragma clang fp contract(off)     // every operation of the rules is a single rounding, or an explicit fmaf

namespace sfm {

// the window of one item: GU x GV cells of side c around (ox, oy) -- the row itself, both sides G; or the vehicle's centre point
struct GridWindow {
    float ox, oy, hx, hy;      // the window's middle in world axes; the heading of frame 1
    float c, halfu, halfv, gu, gv;
    int GU;
    bool rot;
    __device__ __forceinline__ GridWindow(float c_, int GU_, int GV, bool rot_)
        : c(c_), halfu(0.5f * (float)GU_), halfv(0.5f * (float)GV), gu((float)GU_), gv((float)GV), GU(GU_), rot(rot_) {}   // (all exact)
    // the rotation into the heading frame: the rules of include/sfm_hip.h
    __device__ __forceinline__ void rotate(float& a, float& b) const {
        if (rot) {
            const float ra = fmaf(hx, a, hy * b), rb = fmaf(hx, b, -(hy * a));
            a = ra;
            b = rb;
        }
    }
    // the cell [cv][cu] of a source at (px, py), as cv * GU + cu; -1: outside (NaN and +-inf fail the compares)
    __device__ __forceinline__ int cell(float px, float py) const {
        float ax = px - ox, ay = py - oy;
        rotate(ax, ay);
        const float pu = ax / c + halfu;                               // the division is rounded first (correctly: hipcc's default
        const float pv = ay / c + halfv;                               // for fp32 divide), then the sum
        const bool in = pu >= 0.0f && pu < gu && pv >= 0.0f && pv < gv;
        return in ? (int)pv * GU + (int)pu : -1;
    }
};

// A lane owns the cells tid + q BLOCK, q = 0 .. 3, and keeps a count and two sums for each in the named scalars C0 .. C3, X0 .. X3,
// Y0 .. Y3 of the kernel (macros: the accumulators stay plain registers -- a struct of them, or references to them, go to scratch).
// `tid` and `wave` are the kernel's.
// GRID_ADD: one source, in its turn.  Its cell is uniform, so the three waves that do not hold the owning lane pass over it on a
// scalar test.
#define GRID_ADD(cell, v, C, X, Y)                                                                                             \
    do {                                                                                                                       \
        const int cid_ = __builtin_amdgcn_readfirstlane(cell);                                                                 \
        if (((cid_ / WAVE) & (WAVES_PER_BLOCK - 1)) != wave) break; /* uniform: the owning lane sits in another wave */         \
        const bool mine_ = (cid_ & (BLOCK - 1)) == tid;                                                                        \
        const int q_ = cid_ / BLOCK; /* uniform */                                                                             \
        if (q_ == 0) { C##0 += mine_; X##0 = mine_ ? X##0 + (v).x : X##0; Y##0 = mine_ ? Y##0 + (v).y : Y##0; }                \
        else if (q_ == 1) { C##1 += mine_; X##1 = mine_ ? X##1 + (v).x : X##1; Y##1 = mine_ ? Y##1 + (v).y : Y##1; }           \
        else if (q_ == 2) { C##2 += mine_; X##2 = mine_ ? X##2 + (v).x : X##2; Y##2 = mine_ ? Y##2 + (v).y : Y##2; }           \
        else { C##3 += mine_; X##3 = mine_ ? X##3 + (v).x : X##3; Y##3 = mine_ ? Y##3 + (v).y : Y##3; }                        \
    } while (0)
// GRID_WALK: the LDS list {cid[k], rv[k]}, k = 0 .. count-1, in order: ascending k, fp32 adds, no float atomic
#define GRID_WALK(cid, rv, count, C, X, Y)                                                                                     \
    do {                                                                                                                       \
        int k_ = 0;                                                                                                            \
        _Pragma("unroll 1")                                                                                                    \
        for (; k_ + 4 <= (count); k_ += 4) { /* uniform: the LDS reads are broadcasts, four in flight */                       \
            const int e0 = (cid)[k_], e1 = (cid)[k_ + 1], e2 = (cid)[k_ + 2], e3 = (cid)[k_ + 3];                              \
            const float2 v0 = (rv)[k_], v1 = (rv)[k_ + 1], v2 = (rv)[k_ + 2], v3 = (rv)[k_ + 3];                               \
            GRID_ADD(e0, v0, C, X, Y);                                                                                         \
            GRID_ADD(e1, v1, C, X, Y);                                                                                         \
            GRID_ADD(e2, v2, C, X, Y);                                                                                         \
            GRID_ADD(e3, v3, C, X, Y);                                                                                         \
        }                                                                                                                      \
        _Pragma("unroll 1")                                                                                                    \
        for (; k_ < (count); ++k_) {                                                                                           \
            const int e_ = (cid)[k_];                                                                                          \
            const float2 v_ = (rv)[k_];                                                                                        \
            GRID_ADD(e_, v_, C, X, Y);                                                                                         \
        }                                                                                                                      \
    } while (0)
// GRID_OFFER: the candidates lo .. hi-1 in ascending order, BLOCK at a time: source(i, cell, rx, ry) gives the lane's candidate i its
// cell (left at -1: no source) and its relative velocity; the sources are compacted, by ballots and so in ascending i, into the
// kernel's LDS lists sh.cid / sh.rv of LIST entries (whole passes of the workgroup), which are walked whenever LIST candidates have
// been offered and at the end: the order holds at any number of candidates.  Behind the compaction's first barrier everyone is done
// with the list walked before.  `lane` is the kernel's too; every lane of the workgroup comes here.
#define GRID_OFFER(LIST, lo, hi, source, C, X, Y)                                                                              \
    do {                                                                                                                       \
        int n_ = 0, offered_ = 0;                                                                                              \
        _Pragma("unroll 1")                                                                                                    \
        for (int base_ = (lo); base_ < (hi); base_ += BLOCK) { /* uniform */                                                   \
            int cell_ = -1;                                                                                                    \
            float rx_ = 0.0f, ry_ = 0.0f;                                                                                      \
            if (base_ + tid < (hi)) source(base_ + tid, cell_, rx_, ry_);                                                      \
            n_ += block_compact(cell_ >= 0, sh.wcount, lane, wave, n_, [&](int p_) {                                           \
                sh.cid[p_] = (unsigned short)cell_;                                                                            \
                sh.rv[p_] = make_float2(rx_, ry_);                                                                             \
            });                                                                                                                \
            offered_ += BLOCK;                                                                                                 \
            if (offered_ == (LIST) || base_ + BLOCK >= (hi)) { /* uniform: the chunk is full, or the run is over */            \
                GRID_WALK(sh.cid, sh.rv, n_, C, X, Y);                                                                         \
                n_ = 0;                                                                                                        \
                offered_ = 0;                                                                                                  \
            }                                                                                                                  \
        }                                                                                                                      \
    } while (0)

}  // namespace sfm
