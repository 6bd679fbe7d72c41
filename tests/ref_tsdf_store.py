"""The brick store behind the rolling window, restated for the tests (``thor_slam_amd/dense_store.py``
is the product's spec; ``k_tsdf_store_out`` / ``k_tsdf_store_in`` the device code).  Built on
``ref_tsdf_follow.Window``; nothing of the rule is imported from the product.

* window voxel (i, j, k) at cumulative shift sh is absolute voxel a = (i, j, k) + sh, in brick
  floor(a / 8) at local index a mod 8 (Python's ``//`` and ``%``: floor, non-negative remainder);
* a voxel's words: the u32 views of tsdf, weight, [colour weight, colour R G B], [free-space word];
* a move by delta: (1) every voxel whose destination (i, j, k) - delta is outside the volume and
  that has a non-zero word goes to the store (brick allocated if absent; dropped and counted when
  the pool is full or a brick coordinate is outside [-2^20, 2^20)); (2) the layers move;
  (3) every voxel whose source (i, j, k) + delta is outside takes the store's words, which are zeroed;
* content: bricks with a non-zero word, ascending (bz, by, bx).
"""

from __future__ import annotations

import numpy as np

import ref_tsdf_follow as REF

TWO20 = 2 ** 20


class StoreWindow(REF.Window):
    """``layers``: the window's layers in the move's order, e.g. ("tsdf", "weight") or
    ("tsdf", "weight", "color_weight", "color", "freespace").  ``capacity`` None: unbounded.
    ``store`` False: the parent's behaviour (what leaves is dropped), for comparison."""

    def __init__(self, *args, layers=("tsdf", "weight"), capacity=None, store=True, **kw):
        super().__init__(*args, **kw)
        self.layers, self.capacity, self.store_on = tuple(layers), capacity, store
        if "freespace" in self.layers:
            self.vol["freespace"] = np.zeros(self.vol["tsdf"].shape, np.uint32)
        self.clear_store()

    def clear_store(self):
        self.bricks = {}            # (bx, by, bz) -> u32 [C][8][8][8]
        self.dropped = self.n_moves = self.left_nonzero = 0

    # -- the words of the window ---------------------------------------------------------------------
    @property
    def C(self) -> int:
        return sum(3 if k == "color" else 1 for k in self.layers)

    def words(self) -> np.ndarray:
        """u32 [C][nz][ny][nx]"""
        out = []
        for k in self.layers:
            w = np.ascontiguousarray(self.vol[k]).view(np.uint32)
            out += [w[..., c] for c in range(3)] if k == "color" else [w]
        return np.stack(out)

    def set_words(self, W: np.ndarray) -> None:
        c = 0
        for k in self.layers:
            if k == "color":
                self.vol[k] = np.ascontiguousarray(np.moveaxis(W[c:c + 3], 0, -1)).view(np.float32)
                c += 3
            else:
                self.vol[k] = W[c].copy().view(self.vol[k].dtype)
                c += 1

    def _index(self):
        nz, ny, nx = self.vol["tsdf"].shape
        return np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")

    def _outside(self, delta, sign):
        nz, ny, nx = self.vol["tsdf"].shape
        k, j, i = self._index()
        i, j, k = i + sign * delta[0], j + sign * delta[1], k + sign * delta[2]
        return (i < 0) | (i >= nx) | (j < 0) | (j >= ny) | (k < 0) | (k >= nz)

    def _absolute(self, sel):
        k, j, i = self._index()
        a = np.stack([i[sel] + self.shift[0], j[sel] + self.shift[1], k[sel] + self.shift[2]], axis=1)
        return a // 8, a % 8

    # -- the move ------------------------------------------------------------------------------------
    def shift_by(self, delta) -> None:
        delta = tuple(int(d) for d in delta)
        if any(abs(self.shift[a] + delta[a]) >= REF.TWO30 for a in range(3)):
            delta = (0, 0, 0)
        if not self.store_on or not any(delta):
            super().shift_by(delta)
            return
        self.n_moves += 1
        W = self.words()
        sel = self._outside(delta, -1) & W.any(axis=0)
        self.left_nonzero += int(sel.sum())
        b, loc = self._absolute(sel)
        vals = W[:, sel]                                        # [C][n]
        for key in sorted({tuple(r) for r in b.tolist()}, key=lambda r: (r[2], r[1], r[0])):
            m = (b == np.array(key)).all(axis=1)
            if key not in self.bricks:
                if any(not -TWO20 <= c < TWO20 for c in key) or (self.capacity is not None and len(self.bricks) >= self.capacity):
                    self.dropped += int(m.sum())
                    continue
                self.bricks[key] = np.zeros((self.C, 8, 8, 8), np.uint32)
            self.bricks[key][:, loc[m, 2], loc[m, 1], loc[m, 0]] = vals[:, m]
        super().shift_by(delta)
        W = self.words()
        sel = self._outside(delta, +1)
        b, loc = self._absolute(sel)
        idx = np.nonzero(sel)
        for key in {tuple(r) for r in b.tolist()} & set(self.bricks):
            m = (b == np.array(key)).all(axis=1)
            brick = self.bricks[key]
            W[:, idx[0][m], idx[1][m], idx[2][m]] = brick[:, loc[m, 2], loc[m, 1], loc[m, 0]]
            brick[:, loc[m, 2], loc[m, 1], loc[m, 0]] = 0
        self.set_words(W)

    # -- reading ---------------------------------------------------------------------------------------
    def content(self):
        """(bricks i32 [n][3], words u32 [n][C][8][8][8]) in ascending (bz, by, bx)."""
        keys = sorted((k for k, v in self.bricks.items() if v.any()), key=lambda r: (r[2], r[1], r[0]))
        words = np.stack([self.bricks[k] for k in keys]) if keys else np.zeros((0, self.C, 8, 8, 8), np.uint32)
        return np.array(keys, np.int32).reshape(-1, 3), words

    def stats(self) -> dict:
        nonempty = [v for v in self.bricks.values() if v.any()]
        return {"capacity": self.capacity, "bricks_allocated": len(self.bricks), "bricks": len(nonempty),
                "voxels_stored": int(sum(v.any(axis=0).sum() for v in nonempty)), "voxels_dropped": self.dropped,
                "moves": self.n_moves, "words_per_voxel": self.C}

    def assemble(self, lo, hi) -> dict:
        """The layers over the absolute voxel box [lo, hi) (x, y, z) from the window and the store:
        brute force, one dictionary entry per voxel."""
        vox = {}
        for key, brick in self.bricks.items():
            for z, y, x in zip(*np.nonzero(brick.any(axis=0))):
                vox[(8 * key[0] + x, 8 * key[1] + y, 8 * key[2] + z)] = brick[:, z, y, x]
        W = self.words()
        for k, j, i in zip(*np.nonzero(W.any(axis=0))):
            a = (i + self.shift[0], j + self.shift[1], k + self.shift[2])
            assert a not in vox, "a voxel lives in the window or in the store, never in both"
            vox[a] = W[:, k, j, i]
        out = np.zeros((self.C,) + tuple(int(hi[a] - lo[a]) for a in (2, 1, 0)), np.uint32)
        for (x, y, z), w in vox.items():
            if all(lo[a] <= v < hi[a] for a, v in enumerate((x, y, z))):
                out[:, z - lo[2], y - lo[1], x - lo[0]] = w
        res, c = {}, 0
        for k in self.layers:
            if k == "color":
                res[k] = np.ascontiguousarray(np.moveaxis(out[c:c + 3], 0, -1)).view(np.float32)
                c += 3
            else:
                res[k] = out[c].copy().view(np.uint32 if k == "freespace" else np.float32)
                c += 1
        return res
