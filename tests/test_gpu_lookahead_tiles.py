"""GPU parity, PT_LOOKAHEAD in tiled sessions: the contexts of a multi-device session (pt_scene_desc::devices) and the ranks of
the process form (tile_count > 1, PT_SHARED_IMAGE) trace windows of iterations ahead over their own tile, and every call only
gathers its own sample into the rows it owns (csrc/pt_h_api.hpp: la_trace, csrc/pt_k_image.hpp: k_gather_one_tiled,
csrc/pt_multi.hpp: multi_trace).  What the reference's host sees must not change: state.image after EVERY call, the assembled
frame (pt_get_image, pt_device_image) and the statistics equal the oracle's, bit for bit -- across window boundaries, a
skipped iteration number, a camera move, a traceDepth change, pt_clear_image, a batch in between, the calls that fall back
to the plain path (a PBO, a pageable image) and a free / re-init.  Several contexts on device 0 stand in for several GPUs
here: the same code, one tile per context."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402,F401
from gpu_common import pt, launch_plan, bits, _resized  # noqa: E402,F401

pytestmark = pytest.mark.gpu

K = 8                # max_batch: windows of 4, then 8 iterations


def bookkeeping(pt):
    """(windows enqueued, calls that had to trace their own window first, windows discarded -- summed over the contexts --,
    size of the window context 0 is consuming)"""
    out = (C.c_uint64 * 4)()
    assert pt.library().ptdbg_lookahead(out) == 0
    return tuple(int(v) for v in out)


class Oracle:
    """The oracle's running sum, carried across camera / depth changes (as in test_gpu_lookahead.py)."""

    def __init__(self, po, s, cam, depth):
        self.po, self.s = po, s
        self.image = None
        self.rays = 0
        self.retarget(cam, depth)

    def retarget(self, cam, depth):
        t = self.po.Tracer(self.s["geoms"], self.s["materials"], cam, depth, flags=self.po.F_COMPACT, trig=self.po.TRIG_SHARED)
        if self.image is not None:
            t.image[:] = self.image
        self.t, self.image = t, t.image

    def iterate(self, it):
        st = self.t.iterate(it, threads=8)
        self.rays += st.rays
        return self.image


def _device_frame(pt, n):
    """pt_device_image's frame, read through the HIP runtime this process already holds (torch's)."""
    ptr = pt.device_image_ptr()
    assert ptr
    pt.synchronize()
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64.so" in line)
    hip = C.CDLL(path)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.zeros((n, 3), dtype=np.float32)
    assert hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0          # hipMemcpyDeviceToHost
    return out


def _flags(pt):
    return pt.PT_COMPACT | pt.PT_LOOKAHEAD | pt.PT_PIN_IMAGE | pt.PT_HOST_SPARSE


def _drive(pt, po, s, w, h, strip, devices, check_every_call=True):
    """The call sequence of test 1 on a session over `devices` (None: one device, the whole frame).  Returns the
    bookkeeping before the free and the iterations counter after the first call."""
    cam = _resized(s["camera"], w, h)
    n = w * h
    depth = s["depth"]
    scene = pt.Scene(s["geoms"], s["materials"], cam, depth)
    L = pt.library()
    a = np.full((n, 3), -7.0, dtype=np.float32)
    cam2 = cam.copy()
    cam2["position"][0][1] += 0.5
    kw = dict(devices=devices, tile=(0, 1, strip)) if devices else {}
    pt.pathtraceInit(scene, flags=_flags(pt), max_batch=K, pin_image=False, **kw)
    if devices:
        assert pt.num_devices() == len(devices)
    ref = Oracle(po, s, cam, depth)
    first = []

    def call(it, camera=cam, d=depth):
        pt.set_camera(camera, d)                           # the shim forwards both on every pathtrace() (pathtrace.cu:285-286)
        assert L.pt_trace(None, 0, it, a.ctypes.data) == 0, L.pt_last_error()
        want = ref.iterate(it)
        if not first:
            first.append(pt.counters()[2])
        if check_every_call:
            assert (bits(a) == bits(want)).all(), "host image after iteration %d" % it

    for it in range(1, 14):                                # windows [1,4] [5,12], into [13,20]
        call(it)
    assert (bits(pt.get_image(n)) == bits(ref.image)).all()
    call(15)                                               # 14 is skipped
    call(16); call(17)
    ref.retarget(cam2, depth)                              # the camera moves mid-window
    call(18, cam2); call(19, cam2)
    ref.retarget(cam2, depth - 3)                          # traceDepth changes
    for it in range(20, 23):
        call(it, cam2, depth - 3)
    pt.trace_batch(100, 2, None)                           # a batch in between: every context's windows go
    ref.iterate(100); ref.iterate(101)
    call(102, cam2, depth - 3); call(103, cam2, depth - 3)
    pt.clear_image()
    ref.image[:] = 0
    call(104, cam2, depth - 3); call(105, cam2, depth - 3)
    assert (bits(pt.get_image(n)) == bits(ref.image)).all()
    book = bookkeeping(pt)
    pt.pathtraceFree()

    pt.pathtraceInit(scene, flags=_flags(pt), max_batch=K, pin_image=False, **kw)
    ref = Oracle(po, s, cam, depth)
    for it in range(1, 7):
        call(it)
    pt.pathtraceFree()
    return book, first[0]


@pytest.mark.parametrize("devices,w,h,strip", [([0, 0], 400, 300, 8), ([0, 0, 0], 400, 299, 3), ([0, 0, 0, 0], 400, 300, 8)],
                         ids=["2 contexts", "3 contexts, strips of 3 over 299 rows", "4 contexts"])
def test_host_image_after_every_call_equals_the_oracle(pt, po, scenes, launch_plan, devices, w, h, strip):
    _drive(pt, po, scenes["cornell"], w, h, strip, devices)


def test_the_contexts_really_trace_ahead(pt, po, scenes):
    """After the first call every context has traced a window of four (the fallback traces one iteration per call), and the
    bookkeeping of a two-context session is twice that of one device driven the same way: the same windows, misses and
    discards (skipped iteration, camera, depth, batch, pt_clear_image) on each context."""
    s = scenes["cornell"]
    book2, iters2 = _drive(pt, po, s, 400, 300, 8, [0, 0], check_every_call=False)
    book1, iters1 = _drive(pt, po, s, 400, 300, 8, None, check_every_call=False)
    assert iters1 >= 4 and iters2 >= 4
    assert book1[0] > 0 and book1[2] > 0
    assert book2[:3] == tuple(2 * v for v in book1[:3]) and book2[3] == book1[3]


@pytest.mark.parametrize("with_host", [True, False], ids=["host image", "no host image"])
def test_frame_after_lookahead_calls(pt, po, scenes, launch_plan, with_host):
    """pt_get_image and pt_device_image assemble the frame lazily after calls served from the windows (multi_refresh)."""
    s = scenes["cornell"]
    w, h = 400, 299
    cam = _resized(s["camera"], w, h)
    n = w * h
    scene = pt.Scene(s["geoms"], s["materials"], cam, s["depth"])
    L = pt.library()
    a = np.full((n, 3), -7.0, dtype=np.float32)
    pt.pathtraceInit(scene, flags=_flags(pt), max_batch=K, pin_image=False, devices=[0, 0, 0], tile=(0, 1, 5))
    ref = Oracle(po, s, cam, s["depth"])
    for it in range(1, 2 * K + 1):
        assert L.pt_trace(None, 0, it, a.ctypes.data if with_host else None) == 0, L.pt_last_error()
        want = ref.iterate(it)
        if with_host:
            assert (bits(a) == bits(want)).all(), it
        if it % 3 == 0 or it == 2 * K:                     # (every third call: the others run with the device frame stale)
            assert (bits(_device_frame(pt, n)) == bits(want)).all(), it
            assert (bits(pt.get_image(n)) == bits(want)).all(), it
    assert bookkeeping(pt)[1] == 3                         # one miss per context: every call was served from the windows
    pt.pathtraceFree()


def test_fallbacks_stay_exact(pt, po, scenes, launch_plan):
    """A call with a PBO and one with a pageable host image take the plain multi-device path; every context's windows are
    discarded first, every image stays exact, and the next eligible call starts a fresh window."""
    import torch
    s = scenes["cornell"]
    w, h = 400, 300
    cam = _resized(s["camera"], w, h)
    n = w * h
    scene = pt.Scene(s["geoms"], s["materials"], cam, s["depth"])
    L = pt.library()
    pbo = torch.zeros(n * 4, dtype=torch.uint8, device="cuda:0")
    b = np.full((n, 3), -9.0, dtype=np.float32)
    # no PT_PIN_IMAGE: a host image stays pageable, so only the calls without one are served from the windows
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT | pt.PT_LOOKAHEAD | pt.PT_HOST_SPARSE, max_batch=K, pin_image=False,
                     devices=[0, 0], tile=(0, 1, 8))
    ref = Oracle(po, s, cam, s["depth"])
    misses = []
    for it in range(1, 14):
        kind = {6: "pbo", 9: "pageable"}.get(it)
        host = b.ctypes.data if kind == "pageable" else None
        assert L.pt_trace(pbo.data_ptr() if kind == "pbo" else None, 0, it, host) == 0, L.pt_last_error()
        want = ref.iterate(it)
        if kind == "pageable":
            assert (bits(b) == bits(want)).all(), it
        if kind == "pbo":
            assert pbo.cpu().numpy().tobytes() == pt.tonemap(n, it).tobytes(), it
        assert (bits(pt.get_image(n)) == bits(want)).all(), it
        misses.append(bookkeeping(pt)[1])
    # calls 1, 7 and 10 traced a window of their own (after the PBO and the pageable call), on both contexts
    assert misses[0] == 2 and misses[6] == 4 and misses[9] == 6 and misses[-1] == 6
    pt.pathtraceFree()

    # page-locked: a PBO call in the middle of a run of calls with the host image
    a = np.full((n, 3), -7.0, dtype=np.float32)
    pt.pathtraceInit(scene, flags=_flags(pt), max_batch=K, pin_image=False, devices=[0, 0], tile=(0, 1, 8))
    ref = Oracle(po, s, cam, s["depth"])
    for it in range(1, 12):
        with_pbo = it == 6
        assert L.pt_trace(pbo.data_ptr() if with_pbo else None, 0, it, a.ctypes.data) == 0, L.pt_last_error()
        want = ref.iterate(it)
        assert (bits(a) == bits(want)).all(), it
        if with_pbo:
            assert pbo.cpu().numpy().tobytes() == pt.tonemap(n, it).tobytes(), it
    assert bookkeeping(pt)[1] == 4                         # calls 1 and 7, on both contexts
    pt.pathtraceFree()


def test_statistics_add_up(pt, po, scenes):
    """pt_get_stats sums a window's rays once, with the call that starts consuming it: over whole windows the sum is the oracle's."""
    s = scenes["cornell"]
    w, h = 400, 300
    cam = _resized(s["camera"], w, h)
    n = w * h
    scene = pt.Scene(s["geoms"], s["materials"], cam, s["depth"])
    L = pt.library()
    a = np.zeros((n, 3), dtype=np.float32)
    pt.pathtraceInit(scene, flags=_flags(pt), max_batch=K, pin_image=False, devices=[0, 0, 0, 0], tile=(0, 1, 8))
    ref = Oracle(po, s, cam, s["depth"])
    served = 0
    for it in range(1, 21):                                # windows [1,4] [5,12] [13,20], consumed to their ends
        assert L.pt_trace(None, 0, it, a.ctypes.data) == 0, L.pt_last_error()
        ref.iterate(it)
        served += pt.get_stats().rays
    assert (bits(a) == bits(ref.image)).all()
    assert served == ref.rays and served > 0
    pt.pathtraceFree()


def test_process_form_writes_its_own_rows(pt, po, scenes, launch_plan):
    """Two ranks of the process form, one after the other in this process: tile 0 of 2, then tile 1, PT_SHARED_IMAGE |
    PT_LOOKAHEAD into one frame.  Rank 0's calls leave rank 1's rows as they were; after both, the frame is the oracle's."""
    s = scenes["cornell"]
    w, h, strip = 400, 299, 7
    cam = _resized(s["camera"], w, h)
    n = w * h
    scene = pt.Scene(s["geoms"], s["materials"], cam, s["depth"])
    L = pt.library()
    frame = np.full((n, 3), -5.0, dtype=np.float32)
    rows = (np.arange(h) // strip) % 2
    flags = pt.PT_COMPACT | pt.PT_LOOKAHEAD | pt.PT_SHARED_IMAGE
    calls = 12

    pt.pathtraceInit(scene, flags=flags, max_batch=K, tile=(0, 2, strip), pin_image=False)
    ref = Oracle(po, s, cam, s["depth"])
    for it in range(1, calls + 1):
        assert L.pt_trace(None, 0, it, frame.ctypes.data) == 0, L.pt_last_error()
        want = ref.iterate(it).reshape(h, w, 3)
        f = frame.reshape(h, w, 3)
        assert (bits(f[rows == 0]) == bits(want[rows == 0])).all(), it
        assert (f[rows == 1] == -5.0).all(), it
    assert bookkeeping(pt)[:2] == (5, 1)                   # [1,4] and three ahead, [29,36] when [5,12] starts; only call 1 traced its own
    pt.pathtraceFree()

    pt.pathtraceInit(scene, flags=flags, max_batch=K, tile=(1, 2, strip), pin_image=False)
    ref1 = Oracle(po, s, cam, s["depth"])
    for it in range(1, calls + 1):
        assert L.pt_trace(None, 0, it, frame.ctypes.data) == 0, L.pt_last_error()
        want = ref1.iterate(it).reshape(h, w, 3)
        f = frame.reshape(h, w, 3)
        assert (bits(f[rows == 1]) == bits(want[rows == 1])).all(), it
    assert bookkeeping(pt)[1] == 1
    pt.pathtraceFree()
    assert (bits(frame) == bits(ref.image)).all()
