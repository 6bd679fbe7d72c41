"""The brick store behind the dense map's rolling window (``HipSlamConfig.dense_store``;
``tslam_tsdf_store_init`` / ``_stats`` / ``_read``; ``k_tsdf_store_out`` / ``k_tsdf_store_in`` in
``k_tsdf_store.hip``): what leaves the window (``thor_slam_amd/dense_follow.py``) is kept on the
device and comes back when the window returns.  This file is the spec, with a small NumPy model;
``tests/ref_tsdf_store.py`` restates it for the tests.

* **Absolute voxel.**  Window voxel (i, j, k) under the cumulative shift ``sh`` is absolute voxel
  ``a = (i, j, k) + sh``.  It belongs to store brick ``b = floor(a / 8)`` per axis (floor, so
  ``a = -1`` is in brick -1) at local index ``a - 8 b``.  Store bricks are 8 x 8 x 8 voxels; brick
  (0, 0, 0) starts at the unshifted origin ``o0``, so brick b's local voxel (i, j, k) is centred at
  ``o0 + s (8 b + (i, j, k) + 0.5)``.  The grid has nothing to do with the integrator's 16 x 4 x 4
  bricks, and window edges cut store bricks in general.
* **A voxel's words.**  Every 32-bit word of every layer the move moves, in the move's order: tsdf,
  weight, then colour weight and colour (R, G, B) when the colour layer is on, then the free-space
  word when that layer is on: 2, 3, 6 or 7 words.  They are handled as bits.
* **A move by** ``delta`` (the follow decision or ``tslam_tsdf_shift``), store on:

  1. before the move, every window voxel with no place in the moved window — ``(i, j, k) - delta``
     outside the volume; with ``|delta| >= dim`` on an axis that is every voxel — is leaving.  If
     one of its words is non-zero, its words are written to the store at its absolute coordinate,
     and its brick is allocated if absent;
  2. the move runs as without a store;
  3. after it, every window voxel with no source — ``(i, j, k) + delta`` outside the volume — is
     entering: it takes its words from the store if its brick is present (else it stays zero), and
     the stored words are set to zero.

  So a voxel lives in exactly one place: the window and the store never hold the same absolute voxel.
* **Capacity.**  The pool has ``capacity`` bricks, allocated and zeroed by ``tslam_tsdf_store_init``;
  bricks are never freed.  A leaving voxel is dropped, and counted, when no brick can be allocated
  for it or when its brick coordinate lies outside ``[-2^20, 2^20)`` on an axis.  Which new bricks
  win the last free slots of a move is unspecified; everything that is stored is exact.
* **Reading.**  The store's content is the set of bricks with at least one non-zero word, in
  ascending (bz, by, bx).  Slot numbers never leave the library.
* **Reset.**  ``tslam_tsdf_init`` and ``tslam_reset`` empty the store (it stays on);
  ``tslam_tsdf_follow`` leaves it alone; ``tslam_tsdf_write`` / ``_write_color`` act on the window
  only.  The bricks are sized for the layers ``tslam_tsdf_store_init`` finds: it comes after
  ``tslam_tsdf_color`` and ``tslam_tsdf_freespace_init``, and while the store is on the free-space
  layer can be neither added nor freed (``TSLAM_ESTATE``).  The depth archive and the store refuse
  each other, as the archive and following do.

**The mesh of the whole map** (``tslam_mesh_extract_whole``; ``Handle.mesh_whole``;
``HipSlamEngine.get_mesh(whole=True)``; ``k_wmesh_list`` / ``k_wmesh_count`` / ``k_wmesh_emit`` in
``k_tsdf_store_mesh.hip``; the model is ``whole_mesh`` below, ``tests/ref_tsdf_store_mesh.py`` restates
it).  Marching cubes by the rules of ``thor_slam_amd/dense.py``, unchanged — the configuration byte,
``tslam_mc_table.h``, ``t = va / (va - ve)`` in f32, the colour of the nearer voxel — over the
absolute voxel grid above, window and store together, with no seam.

* **A voxel's value.**  Absolute voxel ``a`` takes its (tsdf, weight, colour) from the window when
  ``shift <= a < shift + dims`` on every axis; otherwise from its store brick ``floor(a / 8)`` when
  that brick is present; otherwise it is zero, and so unobserved.  The window and the store never
  hold the same voxel, so there is no precedence to decide.  The free-space word is ignored.
* **A cube** with base corner ``a`` has corners ``a + (n & 1, n >> 1 & 1, n >> 2 & 1)`` and is meshed
  when all 8 have weight >= ``min_weight``.  It belongs to brick ``floor(a / 8)``.
* **A vertex** on the edge from base voxel ``v`` along axis ``ax``: coordinate c is
  ``(float)(o0[c] + s * (v[c] + 0.5))`` in f64, with ``o0`` the configured, unshifted origin and ``v``
  absolute; then ``p[ax] += t * (float)s``.  The position depends on absolute coordinates alone,
  never on where the window stands.  While the shift is zero it equals ``tslam_mesh_extract``'s
  vertex bit for bit; otherwise the two may differ in the last f32 bit, because the window's mesh
  adds ``s * shift`` to the origin first.
* **Order.**  Bricks in ascending (bz, by, bx), the numeric order of ``store_key``; within a brick
  [k][j][i] of the cube's base corner; within a cube table order.  For given map content the output
  is one fixed byte string, wherever the window is.
* **Bricks visited:** every brick the window's extent overlaps, and every stored brick outside that
  range that holds a voxel.  A cube whose base brick is in neither set has an unobserved base corner,
  so these are all that need visiting.  As in the store, a brick whose coordinate lies outside
  ``[-2^20, 2^20)`` on an axis has no key: it is not visited, and not looked up as a source.
* The mesh only reads the store and shares the handle's triangle buffer with ``tslam_mesh_extract``:
  the readers return whichever was extracted last.
"""

from __future__ import annotations

import numpy as np

from .dense import mc_triangle_table
from .dense_follow import LIMIT, move_layer

B = 8                      # TSDF_STORE_B
COORD_LIMIT = 1 << 20      # TSDF_STORE_COORD_LIMIT
LAYER_ORDER = ("tsdf", "weight", "color_weight", "color", "freespace")
STAT_KEYS = ("capacity", "bricks_allocated", "bricks", "voxels_stored", "voxels_dropped", "moves", "words_per_voxel")


def check_store_params(bricks) -> None:
    """``HipSlamConfig.validate`` and the library refuse the same capacity."""
    if isinstance(bricks, bool) or not isinstance(bricks, (int, np.integer)) or not 1 <= bricks <= 1 << 30:
        raise ValueError("dense_store_bricks must be an integer in 1..2^30")


def brick_of(a):
    """(brick, local index) of absolute voxel coordinates (any integer array)."""
    a = np.asarray(a, dtype=np.int64)
    b = np.floor_divide(a, B)
    return b, a - B * b


def words_of(layers: dict) -> np.ndarray:
    """The layers [nz][ny][nx](+[3]) of ``LAYER_ORDER`` that are present, as u32 [C][nz][ny][nx]."""
    out = []
    for key in LAYER_ORDER:
        if key in layers:
            w = np.ascontiguousarray(layers[key]).view(np.uint32)
            out += [w[..., c] for c in range(3)] if key == "color" else [w]
    return np.stack(out)


class Store:
    """The model: ``bricks`` maps (bx, by, bz) to u32 [C][8][8][8] (z, y, x)."""

    def __init__(self, capacity: int | None = None) -> None:
        self.capacity, self.bricks, self.dropped, self.moves = capacity, {}, 0, 0

    def move(self, layers: dict, shift, delta) -> tuple:
        """One move of the window ``layers`` (dict of arrays, replaced in place) at cumulative
        ``shift`` by ``delta``; -> the new shift.  A move that would reach 2^30 moves nothing."""
        shift, delta = [int(v) for v in shift], [int(v) for v in delta]
        if any(abs(shift[a] + delta[a]) >= LIMIT for a in range(3)) or not any(delta):
            return tuple(shift)
        self.moves += 1
        keys = [k for k in LAYER_ORDER if k in layers]
        W = words_of(layers)
        nz, ny, nx = W.shape[1:]
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")

        def outside(sign):
            ii, jj, kk = i + sign * delta[0], j + sign * delta[1], k + sign * delta[2]
            return (ii < 0) | (ii >= nx) | (jj < 0) | (jj >= ny) | (kk < 0) | (kk >= nz)

        # 1. out
        for kk, jj, ii in zip(*np.nonzero(outside(-1) & W.any(axis=0))):
            b, loc = brick_of([ii + shift[0], jj + shift[1], kk + shift[2]])
            key = tuple(int(v) for v in b)
            if key not in self.bricks:
                if any(not -COORD_LIMIT <= v < COORD_LIMIT for v in key) or (
                        self.capacity is not None and len(self.bricks) >= self.capacity):
                    self.dropped += 1
                    continue
                self.bricks[key] = np.zeros((W.shape[0], B, B, B), np.uint32)
            self.bricks[key][:, loc[2], loc[1], loc[0]] = W[:, kk, jj, ii]
        # 2. the move
        for key in keys:
            layers[key] = move_layer(layers[key], delta)
        shift = [shift[a] + delta[a] for a in range(3)]
        # 3. in
        W = words_of(layers).copy()
        for kk, jj, ii in zip(*np.nonzero(outside(+1))):
            b, loc = brick_of([ii + shift[0], jj + shift[1], kk + shift[2]])
            brick = self.bricks.get(tuple(int(v) for v in b))
            if brick is not None:
                W[:, kk, jj, ii] = brick[:, loc[2], loc[1], loc[0]]
                brick[:, loc[2], loc[1], loc[0]] = 0
        c = 0
        for key in keys:
            if key == "color":
                layers[key] = np.stack([W[c + n] for n in range(3)], axis=-1).view(layers[key].dtype)
                c += 3
            else:
                layers[key] = W[c].view(layers[key].dtype)
                c += 1
        return tuple(shift)

    def content(self) -> tuple:
        """(bricks i32 [n][3], words u32 [n][C][8][8][8]) as ``tslam_tsdf_store_read`` gives them."""
        keys = sorted((k for k, v in self.bricks.items() if v.any()), key=lambda b: (b[2], b[1], b[0]))
        c = next(iter(self.bricks.values())).shape[0] if self.bricks else 0
        words = np.stack([self.bricks[k] for k in keys]) if keys else np.zeros((0, c, B, B, B), np.uint32)
        return np.array(keys, dtype=np.int32).reshape(-1, 3), words


def split_words(words: np.ndarray, color: bool, freespace: bool) -> dict:
    """``tslam_tsdf_store_read``'s words u32 [n][C][8][8][8] as named layers: ``tsdf`` / ``weight``
    f32 [n][8][8][8], with colour ``color_weight`` and ``color`` [n][8][8][8][3], with the
    free-space layer its words u32 as ``freespace``."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    if words.shape[1] != 2 + (4 if color else 0) + (1 if freespace else 0):
        raise ValueError(f"{words.shape[1]} words per voxel do not match the layers")
    out = {"tsdf": words[:, 0].view(np.float32), "weight": words[:, 1].view(np.float32)}
    c = 2
    if color:
        out["color_weight"] = words[:, 2].view(np.float32)
        out["color"] = np.ascontiguousarray(np.moveaxis(words[:, 3:6], 1, -1)).view(np.float32)
        c = 6
    if freespace:
        out["freespace"] = words[:, c].copy()
    return out


ASSEMBLE_KEYS = ("tsdf", "weight", "color", "color_weight", "run", "settled")


def assemble(window: dict, store: dict, lo, hi) -> dict:
    """The whole map over the absolute voxel box [lo, hi) (x, y, z; voxel 0 at the unshifted
    origin) as dense arrays [hi_z - lo_z][hi_y - lo_y][hi_x - lo_x](+[3]): every layer that
    ``window`` (a ``get_dense_map()`` result, optionally with ``get_freespace()``'s ``run`` /
    ``settled`` merged in) and ``store`` (a ``get_dense_store()`` result) both hold.  Voxels in
    neither are zero; no voxel is in both."""
    lo, hi = np.array(lo, dtype=np.int64), np.array(hi, dtype=np.int64)
    if (hi <= lo).any():
        raise ValueError("assemble needs lo < hi on every axis")
    out = {}
    for key in ASSEMBLE_KEYS:
        if key not in window or key not in store:
            continue
        win = np.asarray(window[key])
        dst = np.zeros(tuple(int(v) for v in (hi - lo)[::-1]) + win.shape[3:], win.dtype)

        def paste(src, at):
            """src [nz][ny][nx](...) whose voxel (0, 0, 0) is absolute voxel ``at``."""
            n = np.array(src.shape[:3][::-1], dtype=np.int64)
            a, b = np.maximum(at, lo), np.minimum(at + n, hi)
            if (b <= a).any():
                return
            d = tuple(slice(int(a[x] - lo[x]), int(b[x] - lo[x])) for x in (2, 1, 0))
            s = tuple(slice(int(a[x] - at[x]), int(b[x] - at[x])) for x in (2, 1, 0))
            dst[d] = src[s]

        for b, brick in zip(np.asarray(store["bricks"], dtype=np.int64).reshape(-1, 3), np.asarray(store[key])):
            paste(brick, B * b)
        paste(win, np.asarray(window["window_shift"], dtype=np.int64))
        out[key] = dst
    return out


def _coord_ok(b) -> bool:
    return all(-COORD_LIMIT <= int(v) < COORD_LIMIT for v in b)


def whole_mesh(window: dict, store: dict, origin, voxel_size: float, min_weight: float, colors: bool = False):
    """The model of ``tslam_mesh_extract_whole``: ``window`` holds ``tsdf`` / ``weight`` f32
    [nz][ny][nx], ``window_shift`` and, for ``colors``, ``color`` [nz][ny][nx][3]; ``store`` holds
    ``bricks`` i32 [n][3] and ``tsdf`` / ``weight`` [n][8][8][8] (and ``color`` [n][8][8][8][3]), as
    ``get_dense_map()`` and ``get_dense_store()`` give them; ``origin`` is the configured one.
    -> (triangles f32 [m][3][3], colours f32 [m][3][3] or None, bricks visited)."""
    count, table = mc_triangle_table()
    lo = np.array(window["window_shift"], dtype=np.int64)
    names = ("tsdf", "weight") + (("color",) if colors else ())
    win = {k: np.asarray(window[k], np.float32) for k in names}
    dims = np.array(win["tsdf"].shape[::-1], dtype=np.int64)
    stored = {}
    for r, b in enumerate(np.asarray(store["bricks"], dtype=np.int64).reshape(-1, 3)):
        stored[tuple(int(v) for v in b)] = {k: np.asarray(store[k][r], np.float32) for k in names}
    b0, b1 = brick_of(lo)[0], brick_of(lo + dims - 1)[0]
    visit = {(x, y, z) for z in range(int(b0[2]), int(b1[2]) + 1) for y in range(int(b0[1]), int(b1[1]) + 1)
             for x in range(int(b0[0]), int(b1[0]) + 1)}
    visit |= set(stored)                              # the store's content: every brick there holds a voxel
    visit = sorted((b for b in visit if _coord_ok(b)), key=lambda b: (b[2], b[1], b[0]))
    o0, s, sf = [float(v) for v in origin], float(voxel_size), np.float32(voxel_size)
    tz, ty, tx = np.meshgrid(np.arange(9), np.arange(9), np.arange(9), indexing="ij")
    corner = [tuple(slice(d, B + d) for d in (n >> 2 & 1, n >> 1 & 1, n & 1)) for n in range(8)]
    tris, cols = [], []
    for b in visit:
        # the 9 x 9 x 9 corner tile: first the 8 source bricks b + {0, 1}^3 that are present, then,
        # voxel by voxel (a window edge can cut a brick), the window's value wherever the window is
        tile = {k: np.zeros((9, 9, 9) + win[k].shape[3:], np.float32) for k in names}
        for n in range(8):
            bits = (n >> 2 & 1, n >> 1 & 1, n & 1)   # z, y, x
            sb = (b[0] + bits[2], b[1] + bits[1], b[2] + bits[0])
            src = stored.get(sb) if _coord_ok(sb) else None
            if src is not None:
                at = tuple(slice(8, 9) if d else slice(0, 8) for d in bits)
                part = tuple(slice(0, 1) if d else slice(0, 8) for d in bits)
                for k in names:
                    tile[k][at] = src[k][part]
        w = [B * b[0] + tx - lo[0], B * b[1] + ty - lo[1], B * b[2] + tz - lo[2]]
        inwin = np.ones((9, 9, 9), bool)
        for c in range(3):
            inwin &= (w[c] >= 0) & (w[c] < dims[c])
        for k in names:
            tile[k][inwin] = win[k][w[2][inwin], w[1][inwin], w[0][inwin]]
        obs = np.ones((B, B, B), bool)
        cfgs = np.zeros((B, B, B), np.int64)
        for n in range(8):
            obs &= tile["weight"][corner[n]] >= np.float32(min_weight)
            cfgs |= (tile["tsdf"][corner[n]] < 0).astype(np.int64) << n
        cfgs[~obs] = 0
        for k, j, i in zip(*(x.tolist() for x in np.nonzero(count[cfgs]))):   # row-major: [k][j][i]
            cfg = int(cfgs[k, j, i])
            for t in range(int(count[cfg])):
                v, vc = [], []
                for e in table[cfg, t]:
                    ax, m = divmod(int(e), 4)
                    o = [c for c in range(3) if c != ax]
                    off = [0, 0, 0]
                    off[o[0]], off[o[1]] = m & 1, m >> 1
                    base = (i + off[0], j + off[1], k + off[2])
                    end = tuple(base[c] + (c == ax) for c in range(3))
                    va, ve = tile["tsdf"][base[::-1]], tile["tsdf"][end[::-1]]
                    tt = va / (va - ve)                                           # f32
                    p = [np.float32(o0[c] + s * ((B * b[c] + base[c]) + 0.5)) for c in range(3)]
                    p[ax] = p[ax] + tt * sf
                    v.append(p)
                    if colors:
                        vc.append(tile["color"][base[::-1]] if tt < np.float32(0.5) else tile["color"][end[::-1]])
                tris.append(v)
                cols.append(vc)
    out = np.array(tris, dtype=np.float32).reshape(-1, 3, 3)
    return out, (np.array(cols, dtype=np.float32).reshape(-1, 3, 3) if colors else None), len(visit)
