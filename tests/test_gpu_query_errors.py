"""What the twelve query entry points refuse, and in which words.

Per family (closest hit, occlusion, radiance, gather, ambient, probe) and for its host and its
device entry point: the return code and the exact rt_last_error text of every argument error, in
the order the checks are made, and what an empty batch does. Nothing here launches a kernel: every
call either fails its checks or has count == 0.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

from rust_gpu_raytracing_amd import _native as N
from tests.test_gpu_gather import renderer

pytestmark = pytest.mark.gpu

COUNT = 4
CAP = 1 << 24
SENTINEL = 0x5EED5EED5EED


@dataclasses.dataclass(frozen=True)
class Family:
    host: str
    src: str           # the input argument's name in the messages
    dst: str           # the output argument's name
    in_floats: int     # float32 per input record
    out_bytes: int     # per output record
    out_align: int     # what the device entry requires of the output pointer
    shape: str         # "plain": (in, out, count); "path": (..., bounces, first, samples, segments);
                       # "ambient": (..., first, samples)
    cap: int = 0       # the most samples; 0: no cap

    @property
    def device(self):
        return self.host + "_device"

    @property
    def segments(self):
        return self.shape == "path"

    @property
    def samples(self):
        return self.shape != "plain"


FAMILIES = [
    Family("rt_trace_rays", "rays", "hits", 8, 64, 16, "plain"),
    Family("rt_occluded", "rays", "occluded", 8, 1, 1, "plain"),
    Family("rt_radiance", "rays", "radiance", 8, 16, 16, "path"),
    Family("rt_gather", "points", "radiance", 8, 16, 16, "path"),
    Family("rt_ambient", "points", "out", 8, 16, 16, "ambient", CAP),
    Family("rt_probe_sh", "probes", "sh", 4, 144, 16, "path", CAP),
]


def call(lib, ctx, f, entry, src, dst, count=COUNT, samples=1, segments=None):
    P = ctypes.c_void_p
    fn = getattr(lib, entry)
    if f.shape == "plain":
        return fn(ctx, P(src), P(dst), count)
    if f.shape == "ambient":
        return fn(ctx, P(src), P(dst), count, 1, samples)
    if entry == f.host:
        return fn(ctx, P(src), P(dst), count, 2, 1, samples, segments)
    return fn(ctx, P(src), P(dst), count, 2, 1, samples, P(segments))


@pytest.mark.parametrize("f", FAMILIES, ids=[f.host for f in FAMILIES])
def test_refusals_and_empty_batches(gpu, f):
    import torch

    h_in = np.zeros((COUNT, f.in_floats), np.float32)
    h_out = np.zeros(COUNT * f.out_bytes, np.uint8)
    h_seg = ctypes.c_uint64(SENTINEL)
    # device memory with room behind the records, so that the shifted pointers stay inside it
    d_in = torch.zeros(COUNT * f.in_floats + 8, dtype=torch.float32, device=gpu)
    d_out = torch.zeros(COUNT * f.out_bytes + 32, dtype=torch.uint8, device=gpu)
    d_seg = torch.zeros(2, dtype=torch.int64, device=gpu)
    torch.cuda.synchronize(gpu)
    with renderer("c1") as r:
        lib, ctx = r._lib, r._ctx

        def refused(entry, text, *args, **kw):
            assert call(lib, ctx, f, entry, *args, **kw) == N.RT_E_INVALID, (entry, text)
            assert lib.rt_last_error(ctx) == f"{entry}: {text}".encode(), (entry, text, lib.rt_last_error(ctx))

        host_args = (h_in.ctypes.data, h_out.ctypes.data)
        dev_args = (d_in.data_ptr(), d_out.data_ptr())
        seg_ref = ctypes.byref(h_seg) if f.segments else None

        # a NULL context: refused without touching any output
        for entry, args in ((f.host, host_args), (f.device, dev_args)):
            assert call(lib, None, f, entry, *args, count=0, segments=seg_ref if entry == f.host else None) \
                == N.RT_E_INVALID
        assert h_seg.value == SENTINEL

        # the samples checks, before count == 0 and before any pointer check
        if f.samples:
            for entry in (f.host, f.device):
                for count in (COUNT, 0):
                    refused(entry, "samples is 0", None, None, count=count, samples=0)
                    if f.cap:
                        refused(entry, f"samples above {CAP}", None, None, count=count, samples=f.cap + 1)
            assert h_seg.value == SENTINEL
            if f.cap:  # the cap itself is allowed
                assert call(lib, ctx, f, f.host, None, None, count=0, samples=f.cap) == N.RT_OK
                assert call(lib, ctx, f, f.device, None, None, count=0, samples=f.cap) == N.RT_OK

        # count == 0: RT_OK before any pointer check, the error text cleared, *segments = 0 on the host form
        refused(f.host, f"{f.src} or {f.dst} is NULL", None, None)
        assert call(lib, ctx, f, f.host, None, None, count=0, segments=seg_ref) == N.RT_OK
        assert lib.rt_last_error(ctx) == b""
        if f.segments:
            assert h_seg.value == 0
            assert call(lib, ctx, f, f.host, None, None, count=0, segments=None) == N.RT_OK
        assert call(lib, ctx, f, f.device, None, None, count=0, segments=None) == N.RT_OK
        if f.segments:  # (not even the segments pointer is looked at)
            assert call(lib, ctx, f, f.device, None, None, count=0, segments=d_seg.data_ptr() + 4) == N.RT_OK

        # the host form: NULL in, NULL out
        refused(f.host, f"{f.src} or {f.dst} is NULL", None, host_args[1])
        refused(f.host, f"{f.src} or {f.dst} is NULL", host_args[0], None)

        # the device form: NULL in, NULL out (in is looked at first)
        refused(f.device, f"{f.src} is NULL", None, dev_args[1])
        refused(f.device, f"{f.src} is NULL", None, None)
        refused(f.device, f"{f.dst} is NULL", dev_args[0], None)
        # host memory where device memory belongs
        not_device = "must be device memory of the context's device"
        refused(f.device, f"{f.src} {not_device}", host_args[0], dev_args[1])
        refused(f.device, f"{f.dst} {not_device}", dev_args[0], host_args[1])
        if f.segments:
            refused(f.device, f"segments {not_device}", *dev_args, segments=ctypes.addressof(h_seg))
        # misaligned pointers
        refused(f.device, f"{f.src} must be 16-byte aligned", dev_args[0] + 4, dev_args[1])
        if f.out_align > 1:
            refused(f.device, f"{f.dst} must be {f.out_align}-byte aligned", dev_args[0], dev_args[1] + 8)
        if f.segments:
            refused(f.device, "segments must be 8-byte aligned", *dev_args, segments=d_seg.data_ptr() + 4)

        r.synchronize()
    # nothing was written anywhere
    assert not h_out.any() and not bool(d_out.any()) and not bool(d_seg.any())
