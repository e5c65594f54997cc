"""Reference for the motion instance of the temporal stage (rt_denoise_temporal_motion).

Written from the contract text ("THE TEMPORAL STAGE" and "THE MOTION STAGE" in include/rt_abi.h,
the same text as the header comment of rust_gpu_raytracing_amd/csrc/denoise.hip), not from the
kernel: a NumPy float32 restatement in the style of tests/temporal_ref.py, one ufunc per written
operation, skipped taps and static pixels chosen with ``np.where`` -- never multiplied by zero or by
an identity matrix. The filter of step 8 is ``denoise_ref._pass`` with an array-valued ``k_c``.

``TemporalMotionRef`` holds the two history slots (each with or without an I plane) and the
generation rule. ``call`` is a plain rt_denoise_temporal (the slot it writes has no ids),
``call_motion`` an rt_denoise_temporal_motion. Both report the branch counters of
tests/temporal_ref.py; ``call_motion`` adds ``MOTION_COUNTERS``.

Shared by tests/test_temporal_motion_cpu.py and tests/test_gpu_temporal_motion.py.
"""
import numpy as np

from tests import denoise_ref as R
from tests.temporal_ref import COUNTERS, DEFAULTS, EDGE_COUNTERS, _dot3

f32 = np.float32
MOVED, DROP = 1, 2
MOTION_COUNTERS = ("moved_found",   # a pixel with a MOVED record that found history
                   "moved_lost",    # ... that found none although a previous slot exists
                   "static_found",  # a hit pixel without MOVED or DROP that found history
                   "dropped",       # a pixel whose record has DROP (a previous slot exists)
                   "rejected_id",   # a pixel with a tap that passed every test of step 4 and failed the id test
                   "ids_absent")    # a pixel of a motion call whose previous slot has no I plane
MOTION = np.dtype([("m", "<f4", 12), ("normal_scale", "<f4"), ("flags", "<u4"), ("_reserved", "<u4", 2)])


def _table(t):
    return np.zeros(0, MOTION) if t is None else np.ascontiguousarray(t, MOTION).reshape(-1)


class TemporalMotionRef:
    def __init__(self):
        self.slots = [None, None]
        self.cur, self.prev = 0, -1

    def reset(self):
        """rt_temporal_reset."""
        self.slots = [None, None]
        self.prev = -1

    def read(self):
        """rt_read_temporal: (out, n_out) of the last call."""
        s = self.slots[self.cur]
        assert s is not None
        return s["C"], s["Nn"][..., 3]

    def call(self, acc, feats, origin, dirs, k, compute_per_frame, generation, world_to_pixel, **params):
        """One plain rt_denoise_temporal; arguments and result as ``temporal_ref.TemporalRef.call``."""
        return self._call(False, acc, feats, None, origin, dirs, k, compute_per_frame, generation, world_to_pixel,
                          None, None, **params)

    def call_motion(self, acc, feats, ids, origin, dirs, k, compute_per_frame, generation, world_to_pixel,
                    objects=None, spheres=None, **params):
        """One rt_denoise_temporal_motion: ``ids`` (H, W, 2) uint32 is the ID plane, ``objects`` and
        ``spheres`` the motion tables (MOTION arrays or None)."""
        return self._call(True, acc, feats, ids, origin, dirs, k, compute_per_frame, generation, world_to_pixel,
                          objects, spheres, **params)

    def _call(self, motion, acc, feats, ids, origin, dirs, k, compute_per_frame, generation, world_to_pixel,
              objects, spheres, max_history=None, sigma_position=None, normal_min=None, iterations=None,
              sigma_color=None, sigma_albedo=None, sigma_depth=None):
        mh = f32(DEFAULTS["max_history"] if max_history is None else max_history)
        sp = f32(DEFAULTS["sigma_position"] if sigma_position is None else sigma_position)
        nmin = f32(DEFAULTS["normal_min"] if normal_min is None else normal_min)
        it = R.DEFAULTS["iterations"] if iterations is None else int(iterations)
        sc = f32(R.DEFAULTS["sigma_color"] if sigma_color is None else sigma_color)
        sa = f32(R.DEFAULTS["sigma_albedo"] if sigma_albedo is None else sigma_albedo)
        sd = f32(R.DEFAULTS["sigma_depth"] if sigma_depth is None else sigma_depth)
        # the slot rule
        cur, prev = self.cur, self.prev
        if self.slots[cur] is not None and self.slots[cur]["gen"] != generation:
            prev, cur = cur, cur ^ 1
        elif self.slots[cur] is None:
            prev = -1
        P = self.slots[prev] if prev >= 0 else None

        acc = np.asarray(acc)
        assert acc.dtype == f32
        normal, depth = feats["normal"].astype(f32, copy=False), feats["depth"].astype(f32, copy=False)
        albedo, hit_p = feats["albedo"].astype(f32, copy=False), feats["hit"].astype(f32, copy=False)
        o = np.asarray(origin, f32).reshape(3)
        d = np.asarray(dirs, f32).reshape(acc.shape[0], acc.shape[1], 3)
        h, w = depth.shape
        counters = dict.fromkeys(COUNTERS + EDGE_COUNTERS + (MOTION_COUNTERS if motion else ()), 0)
        with np.errstate(all="ignore"):
            # 1. current estimate
            n_samples = f32(np.uint32((int(k) - 1) * int(compute_per_frame) & 0xFFFFFFFF))
            c = acc / n_samples
            hit = hit_p != 0
            # 2. world point
            xp = np.where(hit[..., None], o + d * depth[..., None], d).astype(f32)
            yp, g = xp, normal
            moved = np.zeros((h, w), bool)
            drop = np.zeros((h, w), bool)
            if motion:
                # 2m. record lookup
                ids = np.ascontiguousarray(ids, np.uint32).reshape(h, w, 2)
                kind, index = ids[..., 0], ids[..., 1].astype(np.int64)
                flags = np.zeros((h, w), np.uint32)
                m = np.zeros((h, w, 12), f32)
                ns = np.zeros((h, w), f32)
                for want, table in ((2, _table(objects)), (1, _table(spheres))):
                    if table.shape[0] == 0:
                        continue
                    has = (kind == want) & (index < table.shape[0])
                    rec = table[np.where(has, index, 0)]  # never indexed unclamped
                    flags = np.where(has, rec["flags"], flags)
                    m = np.where(has[..., None], rec["m"], m).astype(f32)
                    ns = np.where(has, rec["normal_scale"], ns).astype(f32)
                drop = (flags & DROP) != 0
                moved = (flags & MOVED) != 0
                ym = np.stack([((m[..., 4 * i] * xp[..., 0] + m[..., 4 * i + 1] * xp[..., 1])
                                + m[..., 4 * i + 2] * xp[..., 2]) + m[..., 4 * i + 3] for i in range(3)], axis=-1)
                gm = np.stack([((m[..., 4 * i] * normal[..., 0] + m[..., 4 * i + 1] * normal[..., 1])
                                + m[..., 4 * i + 2] * normal[..., 2]) * ns for i in range(3)], axis=-1)
                yp = np.where(moved[..., None], ym, xp).astype(f32)
                g = np.where(moved[..., None], gm, normal).astype(f32)
            out, n_out = c, np.full((h, w), n_samples, f32)
            if P is None:
                counters["no_previous"] = h * w
            else:
                M = np.asarray(P["matrix"], f32).reshape(16)
                # 3 / 3m. projection of Y
                ci = {}
                for i in (0, 1, 3):
                    v = (M[i] * yp[..., 0] + M[4 + i] * yp[..., 1]) + M[8 + i] * yp[..., 2]
                    ci[i] = np.where(hit, v + M[12 + i], v).astype(f32)
                fx, fy = ci[0] / ci[3], ci[1] / ci[3]
                on = (ci[3] > 0) & (fx > f32(-1.0)) & (fx < f32(w)) & (fy > f32(-1.0)) & (fy < f32(h))
                on &= ~drop  # a DROP pixel has no history
                counters["off_screen"] = int((~on & ~drop).sum())
                fx, fy = np.where(on, fx, f32(0.0)).astype(f32), np.where(on, fy, f32(0.0)).astype(f32)
                # 4 / 4m. bilinear taps
                x0, y0 = np.floor(fx), np.floor(fy)
                ax, ay = fx - x0, fy - y0
                bx, by = f32(1.0) - ax, f32(1.0) - ay
                ix, iy = x0.astype(np.int64), y0.astype(np.int64)
                f = xp - o
                r2 = _dot3(f, f)
                lim = (sp * sp) * r2
                with_ids = motion and P["I"] is not None
                sw = np.zeros((h, w), f32)
                hn = np.zeros((h, w), f32)
                hc = np.zeros((h, w, 4), f32)
                taps = np.zeros((h, w), np.int64)
                rej_n = np.zeros((h, w), bool)
                rej_p = np.zeros((h, w), bool)
                rej_i = np.zeros((h, w), bool)
                low = np.zeros((h, w), bool)
                high = np.zeros((h, w), bool)
                for qx, qy, wt in ((ix, iy, bx * by), (ix + 1, iy, ax * by), (ix, iy + 1, bx * ay),
                                   (ix + 1, iy + 1, ax * ay)):
                    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    low |= on & (wt > 0) & ((qx < 0) | (qy < 0))
                    high |= on & (wt > 0) & ((qx >= w) | (qy >= h))
                    qxc, qyc = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                    C_q, X_q, Nn_q = P["C"][qyc, qxc], P["X"][qyc, qxc], P["Nn"][qyc, qxc]
                    base = on & inside & (wt > 0) & (X_q[..., 3] == hit_p)
                    ok_n = _dot3(g, Nn_q) >= nmin
                    e = yp - X_q[..., :3]
                    ok_p = _dot3(e, e) <= lim
                    ok_i = (P["I"][qyc, qxc] == ids).all(axis=-1) if with_ids else np.ones((h, w), bool)
                    ok = base & np.where(hit, ok_n & ok_p & ok_i, True)
                    rej_n |= base & hit & ~ok_n
                    rej_p |= base & hit & ok_n & ~ok_p
                    rej_i |= base & hit & ok_n & ok_p & ~ok_i
                    # 5. history sums
                    sw = np.where(ok, sw + wt, sw)
                    hc = np.where(ok[..., None], hc + wt[..., None] * C_q, hc)
                    hn = np.where(ok, hn + wt * Nn_q[..., 3], hn)
                    taps += ok
                have = sw > 0
                hcol = hc / sw[..., None]
                nq = hn / sw
                nh = np.where(nq < mh, nq, mh)
                # 6. blend
                tot = nh + n_samples
                a = n_samples / tot
                blend = hcol + (c - hcol) * a[..., None]
                out = np.where(have[..., None], blend, c).astype(f32)
                n_out = np.where(have, tot, n_out).astype(f32)
                for n in (1, 2, 3, 4):
                    counters[f"taps_{n}"] = int((taps == n).sum())
                counters["rejected_normal"] = int(rej_n.sum())
                counters["rejected_position"] = int(rej_p.sum())
                counters["miss_to_miss"] = int((have & ~hit).sum())
                counters["capped"] = int((have & (nq > mh)).sum())
                counters["outside_low"], counters["outside_high"] = int(low.sum()), int(high.sum())
                if motion:
                    counters["moved_found"] = int((moved & ~drop & have).sum())
                    counters["moved_lost"] = int((moved & ~drop & ~have).sum())
                    counters["static_found"] = int((hit & ~moved & ~drop & have).sum())
                    counters["dropped"] = int(drop.sum())
                    counters["rejected_id"] = int(rej_i.sum())
                    counters["ids_absent"] = 0 if with_ids else h * w
            for arr in (out, n_out, xp):
                assert arr.dtype == f32
            # 7 / 7m. store
            self.slots[cur] = {"C": out, "X": np.concatenate([xp, hit_p[..., None]], axis=-1).astype(f32),
                               "Nn": np.concatenate([normal, n_out[..., None]], axis=-1).astype(f32),
                               "I": ids.copy() if motion else None,
                               "matrix": np.array(world_to_pixel, f32).reshape(16).copy(), "gen": generation}
            self.cur, self.prev = cur, (prev if P is not None else -1)
            # 8. filter
            k_a = f32(1.0) / (sa * sa)
            fc = out
            for i in range(it):
                s_i = sc * f32(0.5 ** i)
                K_i = f32(1.0) / (s_i * s_i)
                k_c = n_out * K_i
                fc = R._pass(fc, normal, depth, albedo, hit_p, 1 << i, k_a, k_c, sd)
                assert fc.dtype == f32
            return {"out": out, "n_out": n_out, "f": fc, "u": R.pack_rgba8(R.clamp01(fc)), "counters": counters}
