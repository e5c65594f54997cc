"""Reference for the temporal stage of the denoiser (rt_denoise_temporal).

Written from the contract in the header comment of rust_gpu_raytracing_amd/csrc/denoise.hip ("THE
TEMPORAL STAGE", the same text as include/rt_abi.h), not from the kernel: a NumPy float32
restatement, one ufunc per written operation (NumPy never fuses a multiply with an add), skipped
taps selected with ``np.where`` -- never multiplied by zero. The filter of step 8 is
``denoise_ref._pass`` with an array-valued ``k_c``.

``TemporalRef`` holds the two history slots and the generation rule; each call also reports how
many pixels took each branch (``COUNTERS``), so that the tests can show their cameras reach all of
them.

Shared by tests/test_temporal_cpu.py and tests/test_gpu_temporal.py.
"""
import numpy as np

from tests import denoise_ref as R

f32 = np.float32
DEFAULTS = dict(max_history=32, sigma_position=0.02, normal_min=0.9)
COUNTERS = ("no_previous",     # there was no previous slot
            "off_screen",      # c_3 <= 0 or the projection fell outside (-1, W) x (-1, H)
            "taps_1", "taps_2", "taps_3", "taps_4",  # that many taps counted
            "rejected_normal",    # a tap inside, w > 0, hit on both sides, failed the normal test
            "rejected_position",  # ... passed the normal test and failed the position test
            "miss_to_miss",       # a miss that found history (a counted tap with hit_q == hit_p == 0)
            "capped")             # hn/sw exceeded max_history
# reported as well, for the tests of frames that are no multiple of the tile: an on-screen pixel with a
# tap of w > 0 off the left or top edge / off the right or bottom edge
EDGE_COUNTERS = ("outside_low", "outside_high")


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


class TemporalRef:
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

    def call(self, acc, feats, origin, dirs, k, compute_per_frame, generation, world_to_pixel, max_history=None,
             sigma_position=None, normal_min=None, iterations=None, sigma_color=None, sigma_albedo=None,
             sigma_depth=None):
        """One rt_denoise_temporal at accumulation generation ``generation``: ``acc`` (H, W, 4) is the
        accumulation, ``feats`` the feature dict, ``origin`` (3,) and ``dirs`` (H, W, 3) the un-jittered
        camera rays, ``world_to_pixel`` the current camera's column-major matrix. Returns a dict:
        out, n_out (the pre-filter blend and the history length), f, u (the filtered f32 and packed
        results) and counters."""
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
        counters = dict.fromkeys(COUNTERS + EDGE_COUNTERS, 0)
        with np.errstate(all="ignore"):
            # 1. current estimate
            n_samples = f32(np.uint32((int(k) - 1) * int(compute_per_frame) & 0xFFFFFFFF))
            c = acc / n_samples
            hit = hit_p != 0
            # 2. world point
            xp = np.where(hit[..., None], o + d * depth[..., None], d).astype(f32)
            out, n_out = c, np.full((h, w), n_samples, f32)
            if P is None:
                counters["no_previous"] = h * w
            else:
                M = np.asarray(P["matrix"], f32).reshape(16)
                # 3. projection
                ci = {}
                for i in (0, 1, 3):
                    v = (M[i] * xp[..., 0] + M[4 + i] * xp[..., 1]) + M[8 + i] * xp[..., 2]
                    ci[i] = np.where(hit, v + M[12 + i], v).astype(f32)
                fx, fy = ci[0] / ci[3], ci[1] / ci[3]
                on = (ci[3] > 0) & (fx > f32(-1.0)) & (fx < f32(w)) & (fy > f32(-1.0)) & (fy < f32(h))
                counters["off_screen"] = int((~on).sum())
                fx, fy = np.where(on, fx, f32(0.0)).astype(f32), np.where(on, fy, f32(0.0)).astype(f32)
                # 4. bilinear taps
                x0, y0 = np.floor(fx), np.floor(fy)
                ax, ay = fx - x0, fy - y0
                bx, by = f32(1.0) - ax, f32(1.0) - ay
                ix, iy = x0.astype(np.int64), y0.astype(np.int64)
                f = xp - o
                r2 = _dot3(f, f)
                lim = (sp * sp) * r2
                sw = np.zeros((h, w), f32)
                hn = np.zeros((h, w), f32)
                hc = np.zeros((h, w, 4), f32)
                taps = np.zeros((h, w), np.int64)
                rej_n = np.zeros((h, w), bool)
                rej_p = np.zeros((h, w), bool)
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
                    ok_n = _dot3(normal, Nn_q) >= nmin
                    e = xp - X_q[..., :3]
                    ok_p = _dot3(e, e) <= lim
                    ok = base & np.where(hit, ok_n & ok_p, True)
                    rej_n |= base & hit & ~ok_n
                    rej_p |= base & hit & ok_n & ~ok_p
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
            for arr in (out, n_out, xp):
                assert arr.dtype == f32
            # 7. store
            self.slots[cur] = {"C": out, "X": np.concatenate([xp, hit_p[..., None]], axis=-1).astype(f32),
                               "Nn": np.concatenate([normal, n_out[..., None]], axis=-1).astype(f32),
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
