"""NumPy restatement of the display contract (rt_display).

Written from the contract in the header comment of rust_gpu_raytracing_amd/csrc/display.hip (the same
text as include/rt_abi.h), not from the kernels: the solve uses Python integers, everything else is
``np.float32``, one ufunc per written operation (NumPy never fuses a multiply with an add).

Shared by tests/test_display_cpu.py and tests/test_gpu_display.py.
"""
import numpy as np

f32 = np.float32
ACCUMULATION, DENOISED, PLANE = 0, 1, 2
LINEAR, REINHARD, ACES = 0, 1, 2
NONE, SRGB = 0, 1
DEFAULTS = dict(source=ACCUMULATION, tone_operator=REINHARD, encode=SRGB, auto_exposure=1, exposure=1.0, key=0.18,
                min_exposure=1.0 / 64.0, max_exposure=64.0, adaptation=1.0, white=4.0, low_permille=100,
                high_permille=50)
T16 = np.array([0x3f800000, 0x3f85aac3, 0x3f8b95c2, 0x3f91c3d3, 0x3f9837f0, 0x3f9ef532, 0x3fa5fed7, 0x3fad583f,
                0x3fb504f3, 0x3fbd08a4, 0x3fc5672a, 0x3fce248c, 0x3fd744fd, 0x3fe0ccdf, 0x3feac0c7, 0x3ff5257d],
               np.uint32).view(f32)


def srgb_table():
    """The table of rt_srgb_table: the IEC 61966-2-1 decode of an 8-bit code in double, rounded to f32."""
    c = np.arange(256, dtype=np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4).astype(f32)


# ------------------------------------------------------------------------------------- 1. metering
def luminance(s):
    s = np.asarray(s, f32)
    return (f32(0.2126) * s[..., 0] + f32(0.7152) * s[..., 1]) + f32(0.0722) * s[..., 2]


def bins_of(lum):
    """(bin, metered) per luminance value."""
    lum = np.asarray(lum, f32)
    with np.errstate(invalid="ignore"):
        metered = (lum > 0) & (lum < np.inf)
    j = (np.ascontiguousarray(lum).view(np.uint32) >> np.uint32(20)).astype(np.int64) - 888
    return np.clip(j, 0, 255), metered


def histogram(s):
    with np.errstate(all="ignore"):
        j, metered = bins_of(luminance(s))
    return np.bincount(j[metered].ravel(), minlength=256).astype(np.uint32)


# ------------------------------------------------------------------------------------- 2. the solve
def solve(hist, key, min_exposure, max_exposure, low_permille, high_permille):
    """None when nothing was metered, else a dict with the integers a, n, q, r and the f32 target E_t."""
    hist = [int(v) for v in hist]
    total = sum(hist)
    if total == 0:
        return None
    lo = total * int(low_permille) // 1000
    hi = total - total * int(high_permille) // 1000
    cum = nn = sn = 0
    for j, c in enumerate(hist):
        n_j = max(0, min(cum + c, hi) - max(cum, lo))
        nn += n_j
        sn += n_j * (2 * j + 1)
        cum += c
    a = (2 * sn + nn) // (2 * nn)
    n = 256 - a
    q = n // 16  # floor
    r = n - 16 * q
    with np.errstate(over="ignore", under="ignore"):
        e_t = f32(key) * np.ldexp(T16[r], q)
        assert e_t.dtype == f32
        e_t = np.minimum(np.maximum(e_t, f32(min_exposure)), f32(max_exposure))
    return dict(a=a, n=n, q=q, r=r, e_t=f32(e_t), total=total)


# ------------------------------------------------------------------------------------- 3. adaptation
def adapt(e_prev, target, min_exposure, max_exposure, adaptation):
    """e_prev: the f32 state or None; target: the f32 E_t or None."""
    if e_prev is None and target is None:
        return np.minimum(np.maximum(f32(1.0), f32(min_exposure)), f32(max_exposure))
    if e_prev is None:
        return f32(target)
    if target is None:
        return f32(e_prev)
    return f32(e_prev) + (f32(target) - f32(e_prev)) * f32(adaptation)


# ------------------------------------------------------------------------------------- 4. tone curve
def tone(c, e, op, white=4.0):
    c = np.asarray(c, f32)
    with np.errstate(all="ignore"):
        x = c * f32(e)
        x = np.where(x > 0, x, f32(0.0)).astype(f32)
        x = np.minimum(x, f32(65536.0))
        if op == REINHARD:
            iw2 = f32(1.0) / (f32(white) * f32(white))
            y = (x * (f32(1.0) + x * iw2)) / (f32(1.0) + x)
        elif op == ACES:
            y = (x * (f32(2.51) * x + f32(0.03))) / (x * (f32(2.43) * x + f32(0.59)) + f32(0.14))
        else:
            assert op == LINEAR
            y = x
        y = np.minimum(y, f32(1.0))
    assert y.dtype == f32
    return y


# ------------------------------------------------------------------------------------- 5. encode
def code_none(y):
    return (np.asarray(y, f32) * f32(255.0)).astype(np.uint32) & np.uint32(0xFF)


def code_srgb(y, table=None):
    """The largest j with table[j] <= y, by the branch-free 8-step search."""
    table = srgb_table() if table is None else table
    y = np.asarray(y, f32)
    j = np.zeros(y.shape, np.int64)
    for step in (128, 64, 32, 16, 8, 4, 2, 1):
        j = j + np.where(table[j + step] <= y, step, 0)
    return j.astype(np.uint32)


def alpha_code(a):
    """clamp01 as the frame's clamp (fmax, fmin: NaN gives 0), then the truncating pack."""
    with np.errstate(all="ignore"):
        a = np.fmin(np.fmax(np.asarray(a, f32), f32(0.0)), f32(1.0))
        return code_none(a)


def pack(s, e, op, encode, white=4.0, table=None):
    """The packed u32 image of source pixels ``s`` (..., 4) at exposure ``e``."""
    s = np.asarray(s, f32)
    y = tone(s[..., :3], e, op, white)
    c = code_srgb(y, table) if encode == SRGB else code_none(y)
    return (c[..., 0] | (c[..., 1] << np.uint32(8)) | (c[..., 2] << np.uint32(16))
            | (alpha_code(s[..., 3]) << np.uint32(24))).astype(np.uint32)


# ------------------------------------------------------------------------------------- a whole call
def display_ref(s, e_prev=None, table=None, **params):
    """One rt_display call on source pixels ``s`` with state ``e_prev`` (None: no state).

    Returns (packed image, exposure used, new state, histogram or None, metered or None); the last two
    are None for a manual call, which leaves the stored ones alone."""
    p = dict(DEFAULTS, **params)
    s = np.asarray(s, f32)
    if p["auto_exposure"]:
        hist = histogram(s)
        sol = solve(hist, p["key"], p["min_exposure"], p["max_exposure"], p["low_permille"], p["high_permille"])
        e = adapt(e_prev, None if sol is None else sol["e_t"], p["min_exposure"], p["max_exposure"], p["adaptation"])
        state, metered = f32(e), int(hist.sum(dtype=np.uint64))
    else:
        e, state, hist, metered = f32(p["exposure"]), e_prev, None, None
    return pack(s, e, p["tone_operator"], p["encode"], p["white"], table), f32(e), state, hist, metered
