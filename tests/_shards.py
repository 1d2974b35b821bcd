"""Helpers of the sharded-path tests.

* ``pack_order``: the row packing of ``sfm_upload_state`` / ``block_plan`` / ``sfm_resort`` restated in NumPy (CPU only).
* ``rows_order``: the caller's index of every row a handle holds, read from its packed rows.
* ``ShardReplay``: G ranks of ``stepper.ShardedStepper``'s protocol replayed in one process, G handles on one GPU; the
  collectives are device copies between the handles' buffers.
* ``oracle_tick``: one CARLA-free tick of the oracle from a merged state (v', x', waypoints, draw counters).
"""
import copy
import math

import numpy as np

TILE = 64
MAX_BLOCKS = 16          # sfm_set_partition: at most 16 blocks
REORDER_MIN_N = 2048     # SFM_REORDER unset: the packing is on from this many pedestrians
DT = 0.05
ARRIVE = 2.0


# ---- the row packing ----------------------------------------------------------------------------------------------
def float_key(v):
    """The order-preserving map float32 -> uint32 of sfm_reorder.hip (-0.0 sorts before +0.0, NaN after +inf)."""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def lround(v):
    """std::lround for the non-negative values used here (half away from zero; NumPy's round is half to even)."""
    return int(math.floor(v + 0.5))


def _clamp_aspect(a):
    return min(max(a, 1.0 / 64.0), 64.0)


def crowd_aspect(x, y):
    """x extent / y extent of the pedestrians with |x|, |y| < 1e12 (parked ones left out), clamped to [1/64, 64]: what
    sfm_upload_state keeps as the handle's pack aspect.  The extents are fp32 differences, as in the library."""
    x = np.asarray(x, dtype=np.float32)
    y = np.asarray(y, dtype=np.float32)
    ok = (np.abs(x) < np.float32(1e12)) & (np.abs(y) < np.float32(1e12))
    if not ok.any():
        return 1.0
    x0, x1, y0, y1 = x[ok].min(), x[ok].max(), y[ok].min(), y[ok].max()
    a = float(np.float32(x1 - x0)) / float(np.float32(y1 - y0)) if (x1 > x0 and y1 > y0) else 1.0
    return _clamp_aspect(a)


def strip_rows(tiles, aspect):
    """Rows per strip for ``tiles`` tiles: about sqrt(tiles * aspect) strips, so that the tiles come out square."""
    n_strips = max(1, min(tiles, lround(math.sqrt(float(tiles) * aspect))))
    return TILE * ((tiles + n_strips - 1) // n_strips)


def block_bounds(n_pad, layout, bounds=None):
    """The block row bounds block_plan uses: the given ones, or the equal split of the padded rows in whole tiles; the last
    bound is at least n_pad."""
    gx, gy = layout
    g = gx * gy
    if bounds is not None and len(bounds) == g + 1:
        b = [int(v) for v in bounds]
    else:
        b = [n_pad * k // g // TILE * TILE for k in range(g + 1)]
    b[0] = 0
    b[g] = max(b[g], n_pad)
    return b


def pack_order(x, y, n_pad, layout=None, bounds=None, aspect=None, reorder=None):
    """perm[s] = the caller's index of the pedestrian at row s, as the library packs the crowd (x, y).

    ``layout`` (gx, gy) and ``bounds`` as given to sfm_set_partition (None: plain strip packing).  ``aspect``: the handle's
    pack aspect -- taken at upload, so a device re-pack of a moved crowd uses the UPLOADED crowd's (None: this crowd's).
    ``reorder`` None: on from N = 2048, as with SFM_REORDER unset.  Stable sorts only: ties keep the order they come in."""
    n = len(x)
    if reorder is None:
        reorder = n >= REORDER_MIN_N
    perm = np.arange(n, dtype=np.int64)
    if not reorder or n == 0:
        return perm
    kx, ky = float_key(x), float_key(y)
    if aspect is None:
        aspect = crowd_aspect(x, y)

    def by(seg, key):
        return seg[np.argsort(key[seg], kind="stable")]

    def strip_pack(r0, r1, rows):
        perm[r0:r1] = by(perm[r0:r1], kx)
        for q in range(r0, r1, rows):
            perm[q:min(r1, q + rows)] = by(perm[q:min(r1, q + rows)], ky)

    gx, gy = layout if layout else (0, 0)
    g = gx * gy
    if g <= 1 or g > MAX_BLOCKS:
        strip_pack(0, n, strip_rows((n + TILE - 1) // TILE, aspect))
        return perm
    b = block_bounds(n_pad, (gx, gy), bounds)
    ba = _clamp_aspect(aspect * gy / gx)                 # a block covers 1/gx of the extent in x and 1/gy in y
    perm[:] = by(perm, kx)
    for c in range(gx):                                  # the column pass: column c is the x ranks of its gy blocks
        c0, c1 = min(n, b[c * gy]), min(n, b[(c + 1) * gy])
        perm[c0:c1] = by(perm[c0:c1], ky)
    for k in range(g):
        r0, r1 = min(n, b[k]), min(n, b[k + 1])
        tiles = max(1, (r1 - r0 + TILE - 1) // TILE)
        strip_pack(r0, r1, strip_rows(tiles, ba))
    return perm


def block_strips(n, n_pad, layout=None, bounds=None, aspect=1.0):
    """[(first row, end row, strip rows)] of every block (one block without a layout), as pack_order cuts them."""
    gx, gy = layout if layout else (0, 0)
    if gx * gy <= 1 or gx * gy > MAX_BLOCKS:
        return [(0, n, strip_rows((n + TILE - 1) // TILE, aspect))]
    b = block_bounds(n_pad, (gx, gy), bounds)
    ba = _clamp_aspect(aspect * gy / gx)
    out = []
    for k in range(gx * gy):
        r0, r1 = min(n, b[k]), min(n, b[k + 1])
        out.append((r0, r1, strip_rows(max(1, (r1 - r0 + TILE - 1) // TILE), ba)))
    return out


# ---- reading a handle's rows --------------------------------------------------------------------------------------
def _xy_keys(x, y):
    xb = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    yb = np.ascontiguousarray(y, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (xb << np.uint64(32)) | yb


def rows_order(rows_xy, loc_xy):
    """Row s -> the caller's index of the pedestrian there, through its (x, y) bits, which must be unique in ``loc_xy``."""
    want = _xy_keys(loc_xy[:, 0], loc_xy[:, 1])
    order = np.argsort(want, kind="stable")
    srt = want[order]
    assert len(np.unique(srt)) == len(srt), "positions are not unique: rows cannot be mapped back"
    got = _xy_keys(rows_xy[:, 0], rows_xy[:, 1])
    at = np.searchsorted(srt, got)
    assert (at < len(srt)).all() and np.array_equal(srt[np.minimum(at, len(srt) - 1)], got), "a row holds no caller's pedestrian"
    return order[at]


def packed_rows(engine, n):
    """(n, 4) float32 {x, y, vx, vy} of a HipShardEngine's packed rows, in its row order (the buffer the next tick reads)."""
    return engine.packed()[0][0].view(-1, 4)[:n].cpu().numpy()


# ---- the oracle ---------------------------------------------------------------------------------------------------
def oracle_tick(loc, vel, wp, draws, sc, vehicles, crossing, prm):
    """One CARLA-free tick from the state (loc, vel, wp (N, 3), draws) and the vehicles the tick sees: v' with its exposure and
    conditioned term sum from the C oracle, then O.free_step's arrival test on the pre-move position and the redraw (its forces
    switched off: they are the C oracle's above).  Returns (v', exposure, absum, waypoints', draws')."""
    from oracle import c_oracle
    from oracle import sfm_oracle as O
    import _parity as P
    geom = O.Geometry(sc.borders, sc.border_centers, sc.border_lengths, sc.static_obstacles, vehicles, sc.dynamic_vel)
    with np.errstate(all="ignore"):
        _, _, v_new, expo, absum = c_oracle.tick(loc, vel, wp, sc.target_speed, sc.radius, crossing, geom, prm, DT,
                                                 theta_tol=P.THETA_TOL)
    expo = expo + P.geometry_tie_exposure(O, loc, vel, wp, sc.target_speed, sc.radius, crossing, geom, prm)
    quiet = copy.copy(prm)
    quiet.enabled = {k: False for k in prm.enabled}
    with np.errstate(all="ignore"):
        _, _, wp_new, draws_new = O.free_step(loc, vel, wp, sc.target_speed, sc.radius, crossing, draws, O.Geometry(), quiet, DT,
                                              ARRIVE, sc.seed, sc.world_side)
    return v_new, expo, absum, wp_new, draws_new


# ---- G ranks in one process -----------------------------------------------------------------------------------------
class ShardReplay:
    """What ``world`` ranks of ShardedStepper do, replayed on one GPU with ``world`` handles (and, ``whole``, one whole-crowd handle
    with the same partition beside them).  Per tick: ``run(1)`` on every rank, or ``begin()`` / exchange / ``end()`` (``split``); the
    exchange copies every rank's own rows [lo, hi) of every ``packed()`` buffer ({x, y, vx, vy} and, 3-D, {z, vz}) into the other
    handles.  Every ``resort_every`` ticks: the ``row_data()`` exchange, ``resort()`` on every handle, then new bounds from
    ``balanced_bounds`` over each rank's ``work()`` -- or, where the ordered kernel measured nothing, over a lopsided cost so that the
    bounds move all the same.  The packing is held to ``pack_order`` at every re-pack.  Needs SFM_RESORT_EVERY=0 in the
    environment: the whole-crowd handle must re-pack when the ranks do, not by itself.

    ``bounds``: explicit row bounds instead of the equal split (they need not be whole tiles: a rank whose rows are not takes the
    ordered kernel); ``partition=False``: no rank blocks, the plain strip packing of an upload; ``resort_every=0``: no re-pack;
    ``dt``, ``redraw``: the ticks' step length and whether they redraw waypoints; ``exchange_buffers``: which of the ``packed()``
    buffers the exchange carries (None: all of them -- anything else computes a wrong crowd, for a test that shows it would be
    noticed); ``recorded_tick()``: a tick that records its forces and does not integrate, on every rank."""

    def __init__(self, cfg, sc, world, layout=None, split=False, resort_every=4, whole=True, bounds=None, partition=True, dt=DT,
                 redraw=True, exchange_buffers=None):
        import torch
        from carla_social_force_model_amd.stepper import HipShardEngine, block_layout, equal_bounds
        self.torch = torch
        self.world, self.split, self.resort_every = world, split, resort_every
        self.redraw, self.exchange_buffers = redraw, exchange_buffers
        self.layout = block_layout(world, layout) if partition else None
        self.ranks = [HipShardEngine(cfg, dt) for _ in range(world)]
        self.whole = HipShardEngine(cfg, dt) if whole else None
        for e in self._handles():
            if self.layout:
                e.set_partition(*self.layout)
            self.n, self.n_pad = e.load(sc)
        self.aspect = crowd_aspect(sc.loc[:, 0], sc.loc[:, 1])        # the handles' pack aspect, fixed at upload
        self.bounds = equal_bounds(self.n, self.n_pad, world) if bounds is None else [int(b) for b in bounds]
        assert len(self.bounds) == world + 1 and self.bounds[0] == 0 and self.bounds[-1] == self.n, self.bounds
        self._apply_bounds()
        self.pending = False
        self.since_resort = 0
        self.repacks = 0
        self.launches = []            # per tick: every rank's launch count (engine.timing()), and whether set_shard came just before
        self.after_set_shard = []
        self.bounds_moved = False

    def _handles(self):
        return self.ranks + ([self.whole] if self.whole else [])

    def _apply_bounds(self):
        self.shard_set = True                              # (set_shard drops geometry forces a rank had launched ahead)
        blocks = self.layout and all(b % TILE == 0 for b in self.bounds[:-1])      # (rank blocks are whole tiles)
        for r, e in enumerate(self.ranks):
            e.set_shard(self.bounds[r], self.bounds[r + 1])
            if blocks:
                e.set_partition(*self.layout, self.bounds)
        if self.whole and blocks:
            self.whole.set_partition(*self.layout, self.bounds)

    def synchronize(self):
        self.torch.cuda.synchronize()

    def exchange(self, buffers_of):
        """every rank's own rows of each buffer into every other rank's copy"""
        self.synchronize()
        bufs = [buffers_of(e) for e in self.ranks]
        for r in range(self.world):
            lo, hi = self.bounds[r], self.bounds[r + 1]
            if hi == lo:
                continue
            for q in range(self.world):
                if q == r:
                    continue
                assert len(bufs[r]) == len(bufs[q])
                for (src, w), (dst, _) in zip(bufs[r], bufs[q]):
                    dst[lo * w:hi * w].copy_(src[lo * w:hi * w])
        self.synchronize()

    def _packed(self, e):
        bufs = e.packed()
        return bufs if self.exchange_buffers is None else [b for k, b in enumerate(bufs) if k in self.exchange_buffers]

    def _flush(self):
        if self.pending:
            self.exchange(self._packed)
            self.pending = False

    def repack(self):
        self._flush()
        self.exchange(lambda e: e.row_data())
        for e in self._handles():
            e.resort()
        self.synchronize()
        self.check_packing()
        costs = [float(e.work()) for e in self.ranks]
        if sum(costs) <= 0.0:                              # the ordered kernel: no measure; a lopsided one moves the bounds anyway
            costs = [float((self.bounds[r + 1] - self.bounds[r]) * (1 + r)) for r in range(self.world)]
        from carla_social_force_model_amd.stepper import balanced_bounds
        new = balanced_bounds(self.bounds, costs, self.n)
        self.bounds_moved |= new != self.bounds
        self.bounds = new
        self._apply_bounds()
        self.since_resort = 0
        self.repacks += 1

    def check_packing(self):
        """After a re-pack every rank holds the same rows, in pack_order of the state for the bounds the re-pack cut at; so does the
        whole-crowd handle, of its own state."""
        rows = [packed_rows(e, self.n) for e in self.ranks]
        for k, r in enumerate(rows[1:], 1):
            assert np.array_equal(r.view(np.uint32), rows[0].view(np.uint32)), f"rank {k} holds another row order than rank 0"
        held = [(rows[0], self.merged()[0])]
        if self.whole:
            held.append((packed_rows(self.whole, self.n), self.whole.engine.state()[0]))
        for k, (r, loc) in enumerate(held):
            got = rows_order(r[:, :2], loc[:, :2])
            want = pack_order(loc[:, 0], loc[:, 1], self.n_pad, self.layout, self.bounds, aspect=self.aspect)
            assert np.array_equal(got, want), (f"re-pack {self.repacks} of the {('ranks', 'whole-crowd handle')[k]}: "
                                               f"{int((got != want).sum())} rows differ from pack_order")

    def tick(self):
        if self.resort_every and self.since_resort >= self.resort_every:
            self.repack()
        if self.split:
            for e in self.ranks:
                e.begin(redraw=self.redraw)
            self._flush()                                  # the previous tick's rows arrive between the two halves
            for e in self.ranks:
                e.end(redraw=self.redraw)
        else:
            self._flush()
            for e in self.ranks:
                e.run(1, redraw=self.redraw)
        self.pending = True
        if self.whole:
            self.whole.run(1, redraw=self.redraw)
        self.synchronize()
        self.launches.append([e.engine.timing()[2] for e in self.ranks])
        self.after_set_shard.append(self.shard_set)
        self.shard_set = False
        self.since_resort += 1

    def recorded_tick(self, which="pedestrian_force"):
        """The exchange, then a tick on every rank that records its forces and does not integrate.  Returns force ``which`` of the
        whole crowd, every pedestrian's from the rank that owns it (no row may be left out, none come from two ranks)."""
        self._flush()
        for e in self.ranks:
            e.engine.tick(record=True)
        self.synchronize()
        got = np.stack([e.engine.forces(which) for e in self.ranks])
        own = ~np.isnan(got[:, :, 0])
        assert (own.sum(axis=0) == 1).all(), "every pedestrian's force must come from exactly one rank"
        return np.choose(np.argmax(own, axis=0)[:, None], list(got))

    def merged(self):
        """(loc, vel, wp, draws) of the whole crowd, every pedestrian from the rank that owns it."""
        got = [e.engine.state() for e in self.ranks]
        draws = [e.engine.draw_counts() for e in self.ranks]
        own = np.stack([~np.isnan(g[0][:, 0]) for g in got])
        assert (own.sum(axis=0) == 1).all(), "every pedestrian must be owned by exactly one rank"
        for r, g in enumerate(got):
            assert own[r].sum() == self.bounds[r + 1] - self.bounds[r], f"rank {r} owns {own[r].sum()} pedestrians"
        loc, vel, wp = (np.choose(np.argmax(own, axis=0)[:, None], [g[k] for g in got]) for k in range(3))
        dr = np.choose(np.argmax(own, axis=0), draws)
        return loc, vel, wp, dr

    def whole_state(self):
        return self.whole.engine.state() + (self.whole.engine.draw_counts(),)

    def vehicles(self):
        return [e.engine.dynamic_obstacles() for e in self.ranks]

    def variants(self):
        """every rank's kernel_variant() (after close(): as they were when it was called)"""
        if getattr(self, "_closed_variants", None) is not None:
            return self._closed_variants
        return [e.engine.kernel_variant() for e in self.ranks]

    def close(self):
        self._closed_variants = self.variants()
        for e in self._handles():
            e.close()
