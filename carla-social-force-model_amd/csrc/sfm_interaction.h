// sfm_interaction.h -- device functions shared by the kernels of sfm_kernels.hip and sfm_batch.hip: the fp32 intrinsics, the
// Moussaid interaction bodies (generic with the reference's exact zero-vector conventions, planar and 3-D fast forms, the
// half-angle theta) and the nearest sampled point of a polyline.  gfx950 (MI355X) only.
#pragma once
#include "sfm_device.h"

namespace sfm {

__device__ __forceinline__ float rsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float uniform(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// ---- the per-pedestrian tick update, shared by the tick kernels of sfm_kernels.hip and sfm_batch.hip ---------------------------
// RSQ picks how 1 / |.| is taken: false -- IEEE sqrt and divide (sfm_tick_kernel, sfm_sym_epilogue_kernel, the batch kernel); true --
// v_rsq_f32, 1 ulp (the fused tick only: ~35 instructions less in front of every workgroup's first systolic step; the zero vector
// still normalises to zero, stateutils.py:85-92, and a pedestrian at rest with target speed 0 still stays at rest,
// stateutils.py:20-23).  Z3: a 3-D crowd; Z3 = false leaves out the z lane (faz = nvz = 0).  sfm_tick_kernel and the batch kernel
// pass Z3 = true for planar crowds too (vz = 0 makes that lane exactly +0): see there why.

// AccelerationForce (forces.py:46-53, stateutils.py:7-15): (ts * unit(w - x) - v) / tau; the desired direction has no z
// (stateutils.py:12-13)
// (P: TickArgs or BatchParams, read where the value is used -- the kernels' scalar loads depend on that order)
template <bool Z3, bool RSQ, class P>
__device__ __forceinline__ void acceleration_force(const P& p, float wx, float wy, float x, float y, float vx, float vy, float vz, float ts,
                                                   float& fax, float& fay, float& faz) {
    const float tx_ = wx - x, ty_ = wy - y;
    float inv;
    if (RSQ) {
        const float n2 = fmaf(tx_, tx_, ty_ * ty_);
        inv = (n2 > 0.0f) ? rsq(n2) : 1.0f;
    } else {
        const float nrm = sqrtf(fmaf(tx_, tx_, ty_ * ty_));
        inv = (nrm == 0.0f) ? 1.0f : 1.0f / nrm;
    }
    fax = (ts * (tx_ * inv) - vx) * p.inv_tau;
    fay = (ts * (ty_ * inv) - vy) * p.inv_tau;
    if (Z3) faz = (0.0f - vz) * p.inv_tau;
}

// calculate_new_velocities + cap_velocity (pedestrian_simulation.py:117-124, stateutils.py:18-23): v + dt F capped at
// ts * max_speed_factor, on the 3-D speed in a 3-D crowd
template <bool Z3, bool RSQ, class P>
__device__ __forceinline__ void capped_velocity(const P& p, float vx, float vy, float vz, float Fx, float Fy, float Fz, float ts,
                                                float& nvx, float& nvy, float& nvz) {
    nvx = fmaf(p.dt, Fx, vx); nvy = fmaf(p.dt, Fy, vy); nvz = Z3 ? fmaf(p.dt, Fz, vz) : 0.0f;
    const float s2 = Z3 ? fmaf(nvx, nvx, fmaf(nvy, nvy, nvz * nvz)) : fmaf(nvx, nvx, nvy * nvy);
    float fac;
    if (RSQ) {
        fac = (s2 > 0.0f) ? fminf(1.0f, (ts * p.max_speed_factor) * rsq(s2)) : 0.0f;   // (speed 0: the capped velocity is 0 whatever the factor)
    } else {
        float sp = sqrtf(s2);
        sp = (sp == 0.0f) ? 1.0f : sp;
        fac = fminf(1.0f, (ts * p.max_speed_factor) / sp);
    }
    nvx *= fac; nvy *= fac; nvz *= fac;
}

// The next waypoint of a pedestrian's counter-based stream: draw `draw` under `key` (SFM_TICK_REDRAW_WAYPOINTS)
__device__ __forceinline__ float2 next_waypoint(uint32_t seed, uint32_t key, uint32_t draw, float side) {
    return make_float2(waypoint_coord(seed, key, draw, 0u, side), waypoint_coord(seed, key, draw, 1u, side));
}

// One wave moves vehicle k by dt * v and regenerates its ring p = c + R(yaw) u (obstacles.py:297-329 without the simulator): the one
// vehicle step of the handle's kernels (sfm_kernels.hip) and the batch kernel (sfm_batch.hip).
__device__ __forceinline__ void advance_vehicle(const DynAdvance& d, int k, int lane, bool advance) {
    float4 c = d.ctr[k];
    if (advance) {
        c.x = fmaf(d.dt, c.z, c.x);
        c.y = fmaf(d.dt, c.w, c.y);
        if (lane == 0) (d.ctr_out ? d.ctr_out : d.ctr)[k] = c;
    }
    const float2 r = d.rot[k];                     // {cos yaw, sin yaw}
    const int o1 = d.off[k + 1];
    float2* pts = d.pts_out ? d.pts_out : d.pts;
    for (int p = d.off[k] + lane; p < o1; p += WAVE) {
        const float2 u = d.local[p];
        pts[p] = make_float2(fmaf(r.x, u.x, fmaf(-r.y, u.y, c.x)), fmaf(r.y, u.x, fmaf(r.x, u.y, c.y)));
    }
}

// One wave writes vehicle k as tick t.tick of its track sees it (sfm_batch_set_vehicle_tracks): a teleport to keyframe
// j = t.tick - first[k] with that keyframe's velocity and yaw (run_simulation.py:56-67, carla_simulation.py:107-111), the ring
// p = c + R(yaw_j) u as advance_vehicle forms it.  Outside 0 <= j < L the vehicle is ABSENT: centre and ring points at +inf, velocity 0
// -- its squared distance to anyone is +inf, which fails every strict-< cull (even against an infinite threshold), and speed 0 never
// makes gap_accepted refuse.  k is wave-uniform, so the track reads are scalar loads.
__device__ __forceinline__ void track_vehicle(const BatchTracks& t, int k, int lane, const int* off, const float2* local, float4* ctr_out,
                                              float2* pts_out) {
    const int e0 = t.off[k];
    const long long j = t.tick - (long long)t.first[k];
    const bool present = j >= 0 && j < (long long)(t.off[k + 1] - e0);
    const float inf = __builtin_inff();
    float4 c = make_float4(inf, inf, 0.0f, 0.0f);
    float2 r = make_float2(1.0f, 0.0f);
    if (present) { c = t.key[e0 + (int)j]; r = t.rot[e0 + (int)j]; }
    if (lane == 0) ctr_out[k] = c;
    const int o1 = off[k + 1];
    for (int p = off[k] + lane; p < o1; p += WAVE) {
        const float2 u = local[p];
        pts_out[p] = present ? make_float2(fmaf(r.x, u.x, fmaf(-r.y, u.y, c.x)), fmaf(r.y, u.x, fmaf(r.x, u.y, c.y))) : make_float2(inf, inf);
    }
}

// One wave moves vehicle k as its command u = {a, b, c, kind} says (sfm_batch_set_vehicle_driving; the caller has found kind 1 or 2,
// k is wave-uniform): the single definition of the rule in include/sfm_hip.h.  Kind 1, velocity: v' = (a, b), the heading turns to
// v' / |v'| unless v' = 0.  Kind 2, unicycle: the heading is turned by the caller's (b, c) = (cos, sin) of this tick's turn and
// normalised again, v' = a h' (a < 0 reverses).  Then centre' = centre + dt v', the ring p = centre' + R(h') u as advance_vehicle forms
// it.  Every line is one correctly rounded fp32 operation or an fmaf.  A vehicle whose centre is not finite stays ABSENT as
// track_vehicle leaves one: centre and ring +inf, velocity 0, the heading kept.  The heading is read from head[k] by every lane and
// stored there by lane 0 of this wave, the only one that touches head[k] in the launch; centre and ring go to the other half.
__device__ __forceinline__ void drive_vehicle(const float4 u, float dt, const float4* ctr, const int* off, const float2* local, float2* head,
                                              float4* ctr_out, float2* pts_out, int k, int lane) {
    const float4 c = ctr[k];
    const float2 h = head[k];
    float hx = h.x, hy = h.y, vx, vy;
    if (u.w == 1.0f) {                                                  // uniform
        const float s2 = fmaf(u.x, u.x, u.y * u.y);
        if (s2 > 0.0f) { const float s = sqrtf(s2); hx = u.x / s; hy = u.y / s; }
        vx = u.x; vy = u.y;
    } else {
        const float gx = fmaf(u.y, h.x, -(u.z * h.y)), gy = fmaf(u.z, h.x, u.y * h.y);
        const float n2 = fmaf(gx, gx, gy * gy);
        if (n2 > 0.0f) { const float n = sqrtf(n2); hx = gx / n; hy = gy / n; }
        vx = u.x * hx; vy = u.x * hy;
    }
    const float inf = __builtin_inff();
    const bool present = fabsf(c.x) < inf && fabsf(c.y) < inf;          // (a NaN fails it)
    float4 o = make_float4(fmaf(dt, vx, c.x), fmaf(dt, vy, c.y), vx, vy);
    if (!present) { o = make_float4(inf, inf, 0.0f, 0.0f); hx = h.x; hy = h.y; }
    if (lane == 0) { ctr_out[k] = o; head[k] = make_float2(hx, hy); }
    const int o1 = off[k + 1];
    for (int p = off[k] + lane; p < o1; p += WAVE) {
        const float2 q = local[p];
        pts_out[p] = present ? make_float2(fmaf(hx, q.x, fmaf(-hy, q.y, o.x)), fmaf(hy, q.x, fmaf(hx, q.y, o.y))) : make_float2(inf, inf);
    }
}

// The tile-box rule (the operands of tiles_negligible): a row counts unless it is parked far away (a despawned pedestrian or
// padding), and its speed bound is rounded up so that it stays a bound.  A tile's box and bound are the union over its rows:
// the callers start from an empty box (+inf / -inf, 0), put in each row that counts, then tile_box_reduce over the wave.
__device__ __forceinline__ bool in_tile_box(float x) { return fabsf(x) < BOX_LIMIT; }
__device__ __forceinline__ float speed_bound(float s2) { return sqrtf(s2) * 1.000001f; }
__device__ __forceinline__ void tile_box_reduce(float& x0, float& y0, float& x1, float& y1, float& v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        x0 = fminf(x0, __shfl_xor(x0, m)); y0 = fminf(y0, __shfl_xor(y0, m));
        x1 = fmaxf(x1, __shfl_xor(x1, m)); y1 = fmaxf(y1, __shfl_xor(y1, m));
        v = fmaxf(v, __shfl_xor(v, m));
    }
}

// atan2(s, c) for (s, c) not both zero; minimax odd polynomial of degree 15 on [0,1]
// (fit error 8.9e-8), octant fix-up by selects.  GUARD handles (0,0) -> 0 like np.arctan2.
template <bool GUARD>
__device__ __forceinline__ float atan2_poly(float s, float c) {
    const float ax = fabsf(c), ay = fabsf(s);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    float r = mn * rcp(mx);
    if (GUARD) r = (mx == 0.0f) ? 0.0f : r;
    const float z = r * r;
    float p = -0.00478021258342167f;
    p = fmaf(p, z, 0.02455628334061523f);
    p = fmaf(p, z, -0.0599035729461461f);
    p = fmaf(p, z, 0.09942682328546971f);
    p = fmaf(p, z, -0.1402939336508994f);
    p = fmaf(p, z, 0.1997137085401642f);
    p = fmaf(p, z, -0.33332093252900674f);
    p = fmaf(p, z, 0.9999999113883665f);
    float phi = p * r;
    phi = (ay > ax) ? (1.57079632679489662f - phi) : phi;
    phi = (c < 0.0f) ? (3.14159265358979324f - phi) : phi;
    return copysignf(phi, s);
}

// atan2(s, c) for a UNIT vector (s, c) (2-D fast path: both directions are normalised), half-angle form:
//   tan(theta/2) = s / (1 + c)  ->  theta = 2 atan(s / (1 + |c|)) for c >= 0, sign(s)*pi - that for c < 0.
// The ratio is in [-1, 1] for every quadrant, so there is no octant swap, and theta = r * P(r^2) keeps
// full RELATIVE precision for small angles (head-on encounters, where the force is largest).
// 8-coefficient minimax fit of 2*atan(r)/r on [0,1], relative error 8.9e-8 (below the 2^-22 rad resolution of
// the angle between two fp32-rounded directions).  (0,0) -> 0.
__device__ __forceinline__ float atan2_unit(float s, float c) {
    const float r = s * rcp(1.0f + fabsf(c));
    const float z = r * r;
    float p = -0.0095607885413262813f;
    p = fmaf(p, z, 0.049113825228842972f);
    p = fmaf(p, z, -0.11980885478692463f);
    p = fmaf(p, z, 0.1988547939908939f);
    p = fmaf(p, z, -0.28058826128196529f);
    p = fmaf(p, z, 0.39942748114880167f);
    p = fmaf(p, z, -0.66664186893326649f);
    p = fmaf(p, z, 1.9999998228145017f);
    const float a = p * r;
    return (c < 0.0f) ? (copysignf(3.14159265358979324f, s) - a) : a;
}

// One Moussaid interaction (forces.py:85-115 / :241-270) without the common factor -A:
//   (dx,dy,dz) = other - self, (dvx,dvy,dvz) = v_self - v_other, rsum = radii to subtract.
// Adds e1*t + g*n to (gx,gy,gz), n = (-t_y, t_x, 0).
// EXACT reproduces the reference's zero-vector conventions (stateutils.normalize's divide-by-1,
// np.arctan2(0,0) = 0, -0/0 = NaN); the fast form differs from it only for coincident pairs, which the
// caller detects through `rinv_out` and recomputes.
template <bool Z3, bool RAD, bool EXACT>
__device__ __forceinline__ void moussaid(const IxConst& c, float dx, float dy, float dz, float dvx,
                                         float dvy, float dvz, float rsum, float& gx, float& gy, float& gz,
                                         float& rinv_out) {
    const float d2 = fmaf(dx, dx, fmaf(dy, dy, Z3 ? fmaf(dz, dz, TINY) : TINY));
    const float rinv = rsq(d2);
    rinv_out = rinv;
    float d = d2 * rinv;
    const float ex = dx * rinv, ey = dy * rinv;
    const float ez = Z3 ? dz * rinv : 0.0f;
    const float Dx = fmaf(c.lam, dvx, ex), Dy = fmaf(c.lam, dvy, ey);
    const float Dz = Z3 ? fmaf(c.lam, dvz, ez) : 0.0f;
    const float D2 = fmaf(Dx, Dx, fmaf(Dy, Dy, Z3 ? fmaf(Dz, Dz, TINY) : TINY));
    const float rD = rsq(D2);
    float Dn = D2 * rD;                        // |D|
    const float tx = Dx * rD, ty = Dy * rD;
    const float tz = Z3 ? Dz * rD : 0.0f;
    float sn, cs, aL;
    if (EXACT) {
        const bool e_flat = (dx == 0.0f) & (dy == 0.0f);             // xy part of e is the zero vector
        const bool t_flat = (Dx == 0.0f) & (Dy == 0.0f);
        const bool coincident = e_flat & (Z3 ? (dz == 0.0f) : true);
        const bool d_zero = t_flat & (Z3 ? (Dz == 0.0f) : true);
        const float exa = e_flat ? 1.0f : ex;                         // arctan2(0,0) = 0 = angle of (1,0)
        const float txa = t_flat ? 1.0f : tx;
        sn = fmaf(txa, ey, -(ty * exa));
        cs = fmaf(txa, exa, ty * ey);
        d = coincident ? 0.0f : d;
        Dn = d_zero ? 0.0f : Dn;
        const float deff = RAD ? d - rsum : d;
        aL = deff * c.c1 * (1.0f / Dn);                               // -d/B*log2e; B = 0 -> -inf or NaN
    } else {
        sn = fmaf(tx, ey, -(ty * ex));                                // sin / cos of angle(e) - angle(t)
        cs = fmaf(tx, ex, ty * ey);
        const float deff = RAD ? d - rsum : d;
        aL = deff * (rD * c.c1);
    }
    // == wrapped atan2 difference (stateutils.py:104-112); planar fast path: (sn, cs) is a unit vector
    const float ang = (EXACT || Z3) ? atan2_poly<EXACT>(sn, cs) : atan2_unit(sn, cs);
    const float theta = fmaf(-c.eg, Dn, ang);                         // forces.py:101
    const float q = Dn * theta;
    const float q2 = q * q;
    const float e1 = ex2(fmaf(q2, c.k1, aL));                         // exp(-d/B - (n' B theta)^2)
    const float e2 = ex2(fmaf(q2, c.k2, aL));                         // exp(-d/B - (n  B theta)^2)
    float g = copysignf(e2, theta);                                   // sign(theta) * e2
    if (EXACT) g = (theta == 0.0f) ? 0.0f : g;                        // np.sign(0) = 0 (forces.py:108)
    gx = fmaf(e1, tx, gx);
    gx = fmaf(-g, ty, gx);
    gy = fmaf(e1, ty, gy);
    gy = fmaf(g, tx, gy);
    if (Z3) gz = fmaf(e1, tz, gz);
}

// The wrapped angle between two planar directions, biased (stateutils.py:104-112, forces.py:94,101), from S = m sin, C = m cos of
// the angle, m > 0 the common scale:  theta = atan2(S, C) - eg Dn.
// Half-angle form: tan(angle / 2) = S / (m + C); with |C| in the denominator the ratio stays in [-1, 1] for every quadrant and
//   angle = 2 atan(r) for C >= 0,  sign(S) pi - 2 atan(r) for C < 0,  r = S / (m + |C|),
// 2 atan(r) = r P(r^2): 8-coefficient minimax fit on [0, 1], relative error 9.9e-8 (below the 2^-22 rad that the angle between two
// fp32-rounded directions resolves), full relative precision for small angles (head-on encounters, where the force is largest).
// Round 4: the C < 0 branch is sign arithmetic instead of v_cmp + v_cndmask (issue cost of that pair on MI355X: 16 cycles, as much as
// 6.7 fmas -- tools/valu_microbench.hip): with s = copysign(1, C) the denominator s (m + |C|) = s m + C hands the ratio the sign that
// the branch would have given 2 atan(r), and what is left of the branch is the constant k = (1 - s) copysign(pi / 2, S) = 0 or
// sign(S) pi, added by the fma that finishes the polynomial.  Same values as the branch (C >= 0: p r + 0; C < 0: sign(S) pi - p |r|..)
// up to the rounding of the denominator; a NaN in m (coincident pair) still comes out as NaN.
__device__ __forceinline__ float half_angle_theta(float S, float C, float m, float eg, float Dn) {
    const float sc = copysignf(1.0f, C);
    const float r = S * rcp(fmaf(sc, m, C));
    const float z = r * r;
    float p = -0.0095607885413262813f;
    p = fmaf(p, z, 0.049113825228842972f);
    p = fmaf(p, z, -0.11980885478692463f);
    p = fmaf(p, z, 0.1988547939908939f);
    p = fmaf(p, z, -0.28058826128196529f);
    p = fmaf(p, z, 0.39942748114880167f);
    p = fmaf(p, z, -0.66664186893326649f);
    p = fmaf(p, z, 1.9999998228145017f);
    const float h = copysignf(1.57079632679489662f, S);
    const float k = fmaf(-eg, Dn, fmaf(-sc, h, h));                    // 0 or sign(S) pi (pi / 2 doubles exactly), minus the bias eps B
    return fmaf(p, r, k);
}

// The same interaction for the symmetric kernel's planar fast path, arranged for the fewest issued instructions:
//   (dx,dy) = other - self and d2 = dx^2 + dy^2 come from the caller (it has already tested d2 against the reach);
//   (wx,wy) = lambda (v_self - v_other) -- both velocities are pre-multiplied by lambda once per tile, so D = w + e is one
//   fma per component and e itself is never formed: sin / cos of the angle come out scaled by d, S = t x (dx,dy) = d sin,
//   C = t . (dx,dy) = d cos, and the half-angle ratio is S / (d + |C|).
// d2 is NOT padded: a coincident pair gives rsq(0) = inf -> d = NaN -> a NaN term, which the epilogue takes as the
// signal to recompute the tile with the exact body (the reference's conventions for zero vectors, forces.py:97,105).
// CUT: once -d/B is known (two of the five transcendentals in), a step whose 64 exponents are ALL below -41 is dropped: both
// exponentials of every lane are then < 2^-41, the term < 2^-40 A (the same policy as the tile and the reach tests, now with the
// pair's actual |D| instead of a speed bound).  A NaN exponent (coincident pair) never counts as small.  Returns false if dropped.
template <bool RAD, bool CUT>
__device__ __forceinline__ bool moussaid_planar(const IxConst& c, float dx, float dy, float d2, float wx, float wy, float rsum,
                                                float& cx, float& cy) {
    const float rinv = rsq(d2);
    const float d = d2 * rinv;
    const float Dx = fmaf(dx, rinv, wx), Dy = fmaf(dy, rinv, wy);
    const float D2 = fmaf(Dx, Dx, fmaf(Dy, Dy, TINY));
    const float rD = rsq(D2);
    const float deff = RAD ? d - rsum : d;
    const float aL = deff * (rD * c.c1);
    if (CUT && !__any(!(aL <= -41.0f))) return false;
    const float Dn = D2 * rD;                                          // |D|
    const float tx = Dx * rD, ty = Dy * rD;
    const float S = fmaf(tx, dy, -(ty * dx));                          // d sin(angle(e) - angle(t))
    const float C = fmaf(tx, dx, ty * dy);                             // d cos
    const float theta = half_angle_theta(S, C, d, c.eg, Dn);          // forces.py:94,101
    const float q = Dn * theta;
    const float q2 = q * q;
    const float e1 = ex2(fmaf(q2, c.k1, aL));
    const float e2 = ex2(fmaf(q2, c.k2, aL));
    const float g = copysignf(e2, theta);
    cx = fmaf(e1, tx, -(g * ty));
    cy = fmaf(e1, ty, g * tx);
    return true;
}

// The same for a 3-D crowd (round 3; pedestrian_state.py:17-19 keeps 3-component positions and velocities and forces.py:75-117
// takes 3-component norms): e, D and t are 3-vectors, the force is f_v t + f_theta n with n = (-t_y, t_x, 0), and the angle is the
// one between the xy-projections of e and t (stateutils.angle_diff_2d uses components 0 and 1 only) -- neither projection is a unit
// vector, so the half-angle ratio is S / (h + |C|) with h = sqrt(S^2 + C^2) (one more rsq).  d2 is the 3-D squared distance.
// Two pedestrians above one another (e_xy = 0) or a vertical D give h = 0 -> rsq(0) = inf -> NaN, the signal for the exact body
// (np.arctan2(0, 0) = 0 there), like a coincident pair in the planar body.
template <bool RAD, bool CUT>
__device__ __forceinline__ bool moussaid_spatial(const IxConst& c, float dx, float dy, float dz, float d2, float wx, float wy, float wz,
                                                 float rsum, float& cx, float& cy, float& cz) {
    const float rinv = rsq(d2);
    const float d = d2 * rinv;
    const float Dx = fmaf(dx, rinv, wx), Dy = fmaf(dy, rinv, wy), Dz = fmaf(dz, rinv, wz);
    const float D2 = fmaf(Dx, Dx, fmaf(Dy, Dy, fmaf(Dz, Dz, TINY)));
    const float rD = rsq(D2);
    const float deff = RAD ? d - rsum : d;
    const float aL = deff * (rD * c.c1);
    if (CUT && !__any(!(aL <= -41.0f))) return false;
    const float Dn = D2 * rD;                                          // |D|
    const float tx = Dx * rD, ty = Dy * rD, tz = Dz * rD;
    const float S = fmaf(tx, dy, -(ty * dx));                          // |t_xy| |d_xy| sin(angle(e_xy) - angle(t_xy))
    const float C = fmaf(tx, dx, ty * dy);                             // ... cos
    const float h2 = fmaf(S, S, C * C);
    const float h = h2 * rsq(h2);
    const float theta = half_angle_theta(S, C, h, c.eg, Dn);          // forces.py:94,101
    const float q = Dn * theta;
    const float q2 = q * q;
    const float e1 = ex2(fmaf(q2, c.k1, aL));
    const float e2 = ex2(fmaf(q2, c.k2, aL));
    const float g = copysignf(e2, theta);
    cx = fmaf(e1, tx, -(g * ty));
    cy = fmaf(e1, ty, g * tx);
    cz = e1 * tz;
    return true;
}

// ---- nearest sampled point of a polyline: np.argmin's first-minimum rule (forces.py:154,228) -------------
// One LANE per pedestrian, the polyline [o0,o1) is wave-uniform.  A trip brings 64 points in with one coalesced
// load (the next trip's load is in flight meanwhile), parks them in the wave's LDS row, and every lane walks them
// through broadcast ds_read_b128 (two points each).  The running minimum is kept per GROUP of 8 points (4 ops
// per distance + one min3 tree + one compare per group instead of a compare-select pair per point); at the end
// of the trip a lane whose minimum moved re-reads its winning group from the row and takes the first slot
// whose distance -- recomputed with the same operations, so bit-identical -- equals the minimum.
// Groups in ascending order with a strict `<`, first equal slot inside the group: np.argmin's first-minimum rule.
// Slots past the end hold copies of the last point (they can tie with it, never beat it, and come later).
// LDS operations of one wave execute in order, so the row needs no barrier.
// An empty polyline yields a far-away sentinel whose force term underflows to exactly 0.
__device__ __forceinline__ float dist2(float x, float y, float px, float py) {
    const float ax = x - px, ay = y - py;
    return fmaf(ax, ax, ay * ay);
}
__device__ __forceinline__ float2 lane_nearest(const float2* __restrict__ pts, int o0, int o1, float x, float y,
                                               float2* __restrict__ row, int lane) {
    float bd = __builtin_inff();
    float2 sp = make_float2(FAR_AWAY, FAR_AWAY);
    if (o1 <= o0) return sp;
    const int last = o1 - 1;
    float2 nxt = pts[min(o0 + lane, last)];
    for (int p = o0; p < o1; p += WAVE) {
        row[lane] = nxt;
        if (p + WAVE < o1) nxt = pts[min(p + WAVE + lane, last)];
        __builtin_amdgcn_wave_barrier();
        const int cnt = min(WAVE, o1 - p);
        int bl = -1;
        auto group = [&](int u8) {
            const float4* q = reinterpret_cast<const float4*>(row + u8);
            const float4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
            const float d0 = dist2(x, y, q0.x, q0.y), d1 = dist2(x, y, q0.z, q0.w);
            const float d2 = dist2(x, y, q1.x, q1.y), d3 = dist2(x, y, q1.z, q1.w);
            const float d4 = dist2(x, y, q2.x, q2.y), d5 = dist2(x, y, q2.z, q2.w);
            const float d6 = dist2(x, y, q3.x, q3.y), d7 = dist2(x, y, q3.z, q3.w);
            const float m = fminf(fminf(fminf(fminf(d0, d1), d2), fminf(fminf(d3, d4), d5)), fminf(d6, d7));
            const bool take = m < bd;
            bd = take ? m : bd;
            bl = take ? u8 : bl;
        };
#pragma unroll
        for (int u8 = 0; u8 < WAVE; u8 += 8)
            if (u8 < cnt) group(u8);                                   // uniform
        if (bl >= 0) {                                                 // this lane's minimum moved: which slot?
            const float4* q = reinterpret_cast<const float4*>(row + bl);
            const float4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
            sp = make_float2(q3.z, q3.w);
            if (dist2(x, y, q3.x, q3.y) == bd) sp = make_float2(q3.x, q3.y);
            if (dist2(x, y, q2.z, q2.w) == bd) sp = make_float2(q2.z, q2.w);
            if (dist2(x, y, q2.x, q2.y) == bd) sp = make_float2(q2.x, q2.y);
            if (dist2(x, y, q1.z, q1.w) == bd) sp = make_float2(q1.z, q1.w);
            if (dist2(x, y, q1.x, q1.y) == bd) sp = make_float2(q1.x, q1.y);
            if (dist2(x, y, q0.z, q0.w) == bd) sp = make_float2(q0.z, q0.w);
            if (dist2(x, y, q0.x, q0.y) == bd) sp = make_float2(q0.x, q0.y);
        }
        __builtin_amdgcn_wave_barrier();
    }
    return sp;
}

// ---- pedestrian modes, waypoint queues and gap acceptance (sfm_mode_kernel / fsm_arrived and the batch kernel's MODES form) ----
__device__ __forceinline__ float2 park_position(uint32_t pid) {      // where a despawned pedestrian waits: a ghost
    return make_float2(FAR_AWAY + FAR_STEP * (float)(pid + 1u), -FAR_AWAY);
}

// PedModeManager._activate_mode (ped_mode_manager.py:49-70): entry action of `m`; returns the new target speed.
__device__ __forceinline__ float fsm_enter(uint8_t m, float target, float initial, float crossing) {
    if (m == MODE_IDLE || m == MODE_CHECKING) return 0.0f;
    if (m == MODE_WALKING) return initial;
    if (m == MODE_CROSSING) return crossing;
    return target;                                                    // ROAD_TO_SIDEWALK keeps the speed
}
// PedModeManager.set_mode (ped_mode_manager.py:37-47): two requests are diverted through an intermediate mode.
__device__ __forceinline__ uint8_t fsm_request(uint8_t cur, uint8_t want) {
    if (cur == MODE_WALKING && want == MODE_CROSSING) return MODE_CHECKING;
    if (cur == MODE_CROSSING && want == MODE_WALKING) return MODE_ROAD_TO_SIDEWALK;
    return want;
}

// Distance from p to the segment a-b (shapely LineString.distance(Point)).
__device__ __forceinline__ float seg_dist(float2 a, float2 b, float2 p) {
    const float abx = b.x - a.x, aby = b.y - a.y;
    const float ab2 = fmaf(abx, abx, aby * aby);
    float t = ab2 > 0.0f ? (fmaf(p.x - a.x, abx, (p.y - a.y) * aby) / ab2) : 0.0f;
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    const float qx = fmaf(t, abx, a.x) - p.x, qy = fmaf(t, aby, a.y) - p.y;
    return sqrtf(fmaf(qx, qx, qy * qy));
}

// check_traffic (check_traffic.py:7-61) in closed form: does any vehicle's extrapolated path cross the
// pedestrian's path while the pedestrian would be there?  true = safe to cross.  The vehicles are ctr[k0 .. k1) ({cx, cy, vx, vy});
// (ext_x, ext_y) is the extent of the crowd's (the scene's) FIRST vehicle.
__device__ bool gap_accepted(const float4* ctr, int k0, int k1, float ext_x, float ext_y, float2 loc, float2 goal, float ped_speed,
                             float margin) {
    if (margin < 0.0f) return true;                                   // crosses without looking (:24)
    if (!(ped_speed > 0.0f)) return true;
    const float rx = goal.x - loc.x, ry = goal.y - loc.y;
    const float time_ped = sqrtf(fmaf(rx, rx, ry * ry)) / ped_speed;
    const float rr = fmaf(rx, rx, ry * ry);
    for (int k = k0; k < k1; ++k) {
        const float4 c = ctr[k];                           // {cx, cy, vx, vy}
        const float sp = sqrtf(fmaf(c.z, c.z, c.w * c.w));
        const float inv = sp == 0.0f ? 1.0f : 1.0f / sp;
        // (sic) every vehicle is offset by the FIRST vehicle's extent, element-wise (check_traffic.py:35-36)
        const float ox = c.z * inv * ext_x, oy = c.w * inv * ext_y;
        const float2 front = make_float2(c.x + ox, c.y + oy), back = make_float2(c.x - ox, c.y - oy);
        const float T = time_ped + margin;
        const float2 vgoal = make_float2(fmaf(c.z, T, front.x), fmaf(c.w, T, front.y));
        // segment loc-goal (p0 + t r) against back-vgoal (q0 + u s)
        const float sx = vgoal.x - back.x, sy = vgoal.y - back.y;
        const float qpx = back.x - loc.x, qpy = back.y - loc.y;
        const float rxs = rx * sy - ry * sx, qpxr = qpx * ry - qpy * rx;
        bool hit = false, is_seg = false;
        float2 h0 = make_float2(0.f, 0.f), h1 = h0;
        if (rxs != 0.0f) {
            const float t = (qpx * sy - qpy * sx) / rxs, u = qpxr / rxs;
            if (t >= 0.0f && t <= 1.0f && u >= 0.0f && u <= 1.0f) { hit = true; h0 = make_float2(fmaf(t, rx, loc.x), fmaf(t, ry, loc.y)); }
        } else if (qpxr == 0.0f && rr > 0.0f) {                       // collinear: overlap interval on the pedestrian's segment
            const float t0 = fmaf(qpx, rx, qpy * ry) / rr, t1 = t0 + fmaf(sx, rx, sy * ry) / rr;
            const float lo = fmaxf(0.0f, fminf(t0, t1)), hi = fminf(1.0f, fmaxf(t0, t1));
            if (lo <= hi) {
                hit = true; is_seg = lo < hi;
                h0 = make_float2(fmaf(lo, rx, loc.x), fmaf(lo, ry, loc.y));
                h1 = make_float2(fmaf(hi, rx, loc.x), fmaf(hi, ry, loc.y));
            }
        } else if (rr == 0.0f) {                                      // the pedestrian stands on its waypoint: a point against the path
            const float ss = fmaf(sx, sx, sy * sy), w = -fmaf(qpx, sx, qpy * sy);      // w = (loc - back) . s
            if (ss > 0.0f ? (qpx * sy - qpy * sx == 0.0f && w >= 0.0f && w <= ss) : (qpx == 0.0f && qpy == 0.0f)) { hit = true; h0 = loc; }
        }
        if (!hit || sp == 0.0f) continue;
        if (!is_seg) h1 = h0;
        const float tti_ped = seg_dist(h0, h1, loc) / ped_speed;
        const float tti_front = seg_dist(h0, h1, front) / sp, tti_back = seg_dist(h0, h1, back) / sp;
        if (tti_front - margin < tti_ped && tti_ped < tti_back + margin) return false;
    }
    return true;
}

}  // namespace sfm
