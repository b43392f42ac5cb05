"""-m gpu: what the three images of the most recently staged frame answer, in every state a host can meet them in.

The hdr (RGBA32F), sky (RGBA16F) and display (RGBA8) images are each reached by a blocking read, an asynchronous read that
returns a ticket, and a device pointer.  This file pins the return code of all nine in five states - nothing rendered, rendered
but not resolved, resolved, rendered again after the resolve (stale), resolved with an unusable destination - for four ctx
forms: one engine, one engine that is a row partition (the display pass refuses it), two partitions gathered to the root, and
the same with BHRAY_F_GATHER_SKY.  EXPECTED was recorded from the commit BEFORE the nine entry points of either layer were
folded into one image description and three bodies; it is the characterisation that fold had to keep, cell for cell.

In the resolved state the three access forms must deliver the same bytes, and a pitch wider than a row the same rows as a
tight one.  Tickets count up by one per successful asynchronous read; a refused call takes none; a ticket never issued is
BHRAY_E_INVALID.

The one thing that moved with the fold: bhray_read_hdr_async and bhray_read_sky_async with an unusable destination refuse
BEFORE they launch a partly filled batch (the code they return is the earlier one).  The last test here holds that, through the
trace-launch total of bhray_get_level_grids."""
import ctypes as C

import numpy as np
import pytest

import bhusie_amd as B
from tests import common as T

pytestmark = pytest.mark.gpu

OK, E_INVALID, E_STATE = 0, -1, -5
KINDS = {"hdr": 16, "sky": 8, "display": 4}                      # bytes per pixel
FORMS = {
    "engine": dict(device=0),
    "partition": dict(device=0, row_world=2, row_rank=0),         # BHRAY_GATHER_NONE: 27 of the 40 rows
    "gathered": dict(devices=[0, 0]),
    "gathered_sky": dict(devices=[0, 0], gather_sky=True),
}
PAD = 64                                                          # the over-wide pitch: a row and 64 bytes

# fmt: off
EXPECTED = {
    "engine": {
        "empty": {"hdr.async": -5, "hdr.ptr": 0, "hdr.read": 0, "sky.async": -5, "sky.ptr": -5, "sky.read": -5, "display.async": -5, "display.ptr": -5, "display.read": -5},
        "rendered": {"hdr.async": 0, "hdr.ptr": 0, "hdr.read": 0, "sky.async": -5, "sky.ptr": -5, "sky.read": -5, "display.async": -5, "display.ptr": -5, "display.read": -5},
        "resolved": {"resolve_sky": 0, "resolve_display": 0, "hdr.async": 0, "hdr.ptr": 0, "hdr.read": 0, "hdr.async.null": -1, "hdr.async.short": -1, "hdr.async.wide": 0, "hdr.read.null": -1, "hdr.read.short": -1, "hdr.read.wide": 0, "sky.async": 0, "sky.ptr": 0, "sky.read": 0, "sky.async.null": -1, "sky.async.short": -1, "sky.async.wide": 0, "sky.read.null": -1, "sky.read.short": -1, "sky.read.wide": 0, "display.async": 0, "display.ptr": 0, "display.read": 0, "display.async.null": -1, "display.async.short": -1, "display.async.wide": 0, "display.read.null": -1, "display.read.short": -1, "display.read.wide": 0},
        "stale": {"hdr.async": 0, "hdr.ptr": 0, "hdr.read": 0, "sky.async": -5, "sky.ptr": -5, "sky.read": -5, "display.async": -5, "display.ptr": -5, "display.read": -5},
    },
    "partition": {
        "empty": {"hdr.async": -5, "hdr.ptr": 0, "hdr.read": 0, "sky.async": -5, "sky.ptr": -5, "sky.read": -5, "display.async": -5, "display.ptr": -5, "display.read": -5},
        "rendered": {"hdr.async": 0, "hdr.ptr": 0, "hdr.read": 0, "sky.async": -5, "sky.ptr": -5, "sky.read": -5, "display.async": -5, "display.ptr": -5, "display.read": -5},
        "resolved": {"resolve_sky": 0, "resolve_display": -5, "hdr.async": 0, "hdr.ptr": 0, "hdr.read": 0, "hdr.async.null": -1, "hdr.async.short": -1, "hdr.async.wide": 0, "hdr.read.null": -1, "hdr.read.short": -1, "hdr.read.wide": 0, "sky.async": 0, "sky.ptr": 0, "sky.read": 0, "sky.async.null": -1, "sky.async.short": -1, "sky.async.wide": 0, "sky.read.null": -1, "sky.read.short": -1, "sky.read.wide": 0, "display.async": -5, "display.ptr": -5, "display.read": -5, "display.async.null": -5, "display.async.short": -5, "display.async.wide": -5, "display.read.null": -5, "display.read.short": -5, "display.read.wide": -5},
        "stale": {"hdr.async": 0, "hdr.ptr": 0, "hdr.read": 0, "sky.async": -5, "sky.ptr": -5, "sky.read": -5, "display.async": -5, "display.ptr": -5, "display.read": -5},
    },
    "gathered": {
        "empty": {"hdr.async": -5, "hdr.ptr": 0, "hdr.read": -5, "sky.async": -5, "sky.ptr": -5, "sky.read": -5, "display.async": -5, "display.ptr": -5, "display.read": -5},
        "rendered": {"hdr.async": 0, "hdr.ptr": 0, "hdr.read": 0, "sky.async": -5, "sky.ptr": -5, "sky.read": -5, "display.async": -5, "display.ptr": -5, "display.read": -5},
        "resolved": {"resolve_sky": 0, "resolve_display": 0, "hdr.async": 0, "hdr.ptr": 0, "hdr.read": 0, "hdr.async.null": -1, "hdr.async.short": -1, "hdr.async.wide": 0, "hdr.read.null": -1, "hdr.read.short": -1, "hdr.read.wide": 0, "sky.async": 0, "sky.ptr": 0, "sky.read": 0, "sky.async.null": -1, "sky.async.short": -1, "sky.async.wide": 0, "sky.read.null": -1, "sky.read.short": -1, "sky.read.wide": 0, "display.async": 0, "display.ptr": 0, "display.read": 0, "display.async.null": -1, "display.async.short": -1, "display.async.wide": 0, "display.read.null": -1, "display.read.short": -1, "display.read.wide": 0},
        "stale": {"hdr.async": 0, "hdr.ptr": 0, "hdr.read": 0, "sky.async": -5, "sky.ptr": -5, "sky.read": -5, "display.async": -5, "display.ptr": -5, "display.read": -5},
    },
    "gathered_sky": {
        "empty": {"hdr.async": -5, "hdr.ptr": -5, "hdr.read": -5, "sky.async": -5, "sky.ptr": 0, "sky.read": 0, "display.async": -5, "display.ptr": -5, "display.read": -5},
        "rendered": {"hdr.async": -5, "hdr.ptr": -5, "hdr.read": -5, "sky.async": 0, "sky.ptr": 0, "sky.read": 0, "display.async": -5, "display.ptr": -5, "display.read": -5},
        "resolved": {"resolve_sky": 0, "resolve_display": 0, "hdr.async": -5, "hdr.ptr": -5, "hdr.read": -5, "hdr.async.null": -5, "hdr.async.short": -5, "hdr.async.wide": -5, "hdr.read.null": -5, "hdr.read.short": -5, "hdr.read.wide": -5, "sky.async": 0, "sky.ptr": 0, "sky.read": 0, "sky.async.null": -1, "sky.async.short": -1, "sky.async.wide": 0, "sky.read.null": -1, "sky.read.short": -1, "sky.read.wide": 0, "display.async": 0, "display.ptr": 0, "display.read": 0, "display.async.null": -1, "display.async.short": -1, "display.async.wide": 0, "display.read.null": -1, "display.read.short": -1, "display.read.wide": 0},
        "stale": {"hdr.async": -5, "hdr.ptr": -5, "hdr.read": -5, "sky.async": 0, "sky.ptr": 0, "sky.read": 0, "display.async": -5, "display.ptr": -5, "display.read": -5},
    },
}
COMPARED = {"engine": ["hdr", "sky", "display"], "partition": ["hdr", "sky"], "gathered": ["hdr", "sky", "display"], "gathered_sky": ["sky", "display"]}
# fmt: on


def _open(form, **kw):
    cfg = B.ladder_from_base((24, 14), 3, 2)                      # 70 x 40: the smallest ladder whose frame admits the display pass
    rp = B.RayPass(cfg, frames_in_flight=1, **FORMS[form], **kw)
    rp.set_textures(*T.textures())
    rp.set_uniforms(*T.uniforms(integration_method=0))
    return rp


class _Probe:
    """The nine entry points on one ctx, with the ticket bookkeeping: every successful asynchronous read must return the next number."""

    def __init__(self, rp):
        self.rp, self.L, self.h = rp, B.lib(), rp._h
        self.W, self.H = rp.frame_size
        self.issued = 0
        self.hip = C.CDLL("libamdhip64.so")
        self.pinned = {k: B.PinnedFrame(self.H, self.W + PAD // bpp, channels16=(k == "sky"), rgba8=(k == "display")) for k, bpp in KINDS.items()}

    def close(self):
        for b in self.pinned.values():
            b.free()
        self.rp.close()

    def rows(self, kind):
        return self.H if kind == "display" else int(self.L.bhray_local_rows(self.h))

    def read(self, kind, dst, pitch):
        return int(getattr(self.L, f"bhray_read_{kind}")(self.h, C.c_void_p(dst), pitch))

    def read_async(self, kind, dst, pitch):
        t = C.c_uint64(1 << 40)
        rc = int(getattr(self.L, f"bhray_read_{kind}_async")(self.h, C.c_void_p(dst), pitch, C.byref(t)))
        if rc == OK:
            assert t.value == self.issued, (kind, t.value, self.issued)          # a refused call in between took no ticket
            self.issued += 1
            assert self.L.bhray_wait_read(self.h, C.c_uint64(t.value)) == OK
        return rc

    def ptr(self, kind):
        p, n = C.c_void_p(), C.c_size_t()
        rc = int(getattr(self.L, f"bhray_{kind}_device_ptr")(self.h, C.byref(p), C.byref(n)))
        return rc, p.value, int(n.value)

    def nine(self):
        """{cell: return code} of the nine entry points with a usable, tight destination"""
        out = {}
        for kind, bpp in KINDS.items():
            host = np.zeros(self.H * self.W * bpp, np.uint8)
            out[f"{kind}.read"] = self.read(kind, host.ctypes.data, self.W * bpp)
            out[f"{kind}.async"] = self.read_async(kind, self.pinned[kind].ptr, self.W * bpp)
            out[f"{kind}.ptr"] = self.ptr(kind)[0]
        return out

    def bad_destinations(self):
        """... with a NULL destination, a pitch one byte short of a row, and a pitch 64 bytes over; the last delivers the tight read's rows"""
        out = {}
        for kind, bpp in KINDS.items():
            rowb, n = self.W * bpp, self.rows(kind)
            tight = np.zeros((self.H, rowb), np.uint8)
            have = self.read(kind, tight.ctypes.data, rowb) == OK
            host = np.full((self.H, rowb + PAD), 0xA5, np.uint8)
            pin = self.pinned[kind].array.view(np.uint8).reshape(self.H, rowb + PAD)
            for access, call, buf in (("read", self.read, host), ("async", self.read_async, pin)):
                out[f"{kind}.{access}.null"] = call(kind, None, rowb)
                out[f"{kind}.{access}.short"] = call(kind, buf.ctypes.data, rowb - 1)
                buf[...] = 0xA5
                out[f"{kind}.{access}.wide"] = rc = call(kind, buf.ctypes.data, rowb + PAD)
                if rc == OK and have:
                    assert np.array_equal(buf[:n, :rowb], tight[:n]), (kind, access)
                    assert (buf[:, rowb:] == 0xA5).all(), (kind, access)             # nothing lands between the rows
        return out

    def same_bytes(self):
        """resolved state: blocking read, asynchronous read and a plain hipMemcpy from the device pointer agree, wherever all three are given"""
        compared = []
        for kind, bpp in KINDS.items():
            rowb, n = self.W * bpp, self.rows(kind)
            a = np.zeros((self.H, rowb), np.uint8)
            pin = self.pinned[kind].array.view(np.uint8).reshape(-1)[: self.H * rowb].reshape(self.H, rowb)
            pin[...] = 0
            rcs = self.read(kind, a.ctypes.data, rowb), self.read_async(kind, pin.ctypes.data, rowb), self.ptr(kind)
            if rcs[0] != OK or rcs[1] != OK or rcs[2][0] != OK:
                continue
            _, p, nbytes = rcs[2]
            assert nbytes == n * rowb and p, (kind, nbytes)
            d = np.zeros((self.H, rowb), np.uint8)
            assert self.hip.hipMemcpy(C.c_void_p(d.ctypes.data), C.c_void_p(p), C.c_size_t(nbytes), 2) == 0      # hipMemcpyDeviceToHost; the blocking read synchronised
            assert np.array_equal(a[:n], pin[:n]) and np.array_equal(a[:n], d[:n]), kind
            assert a[:n].any(), kind
            compared.append(kind)
        return compared


def observe(form):
    """The table of one ctx form: {state: {cell: return code}}, and the kinds whose bytes were compared in the resolved state."""
    P = _Probe(_open(form))
    L, h = P.L, P.h
    table = {}
    assert L.bhray_wait_read(h, C.c_uint64(0)) == E_INVALID                           # no ticket has been issued
    table["empty"] = P.nine()
    P.rp.render()
    table["rendered"] = P.nine()
    resolved = {"resolve_sky": int(L.bhray_resolve_sky(h)), "resolve_display": int(L.bhray_resolve_display(h))}
    resolved.update(P.nine())
    compared = P.same_bytes()
    resolved.update(P.bad_destinations())
    table["resolved"] = resolved
    P.rp.set_uniforms(*T.uniforms(integration_method=0, time=0.5))
    P.rp.render()
    table["stale"] = P.nine()
    assert P.issued > 0
    assert L.bhray_wait_read(h, C.c_uint64(P.issued)) == E_INVALID                    # the next ticket does not exist yet
    assert L.bhray_wait_read(h, C.c_uint64(P.issued - 1)) == OK
    P.close()
    return table, compared


@pytest.mark.parametrize("form", list(FORMS))
def test_return_codes_bytes_and_tickets(form):
    table, compared = observe(form)
    for state, cells in table.items():
        print(form, state, cells)
    assert table == EXPECTED[form]
    assert compared == COMPARED[form]


@pytest.mark.parametrize("form,kind", [("engine", "hdr"), ("gathered", "hdr"), ("gathered_sky", "sky")])
def test_a_refused_async_read_leaves_the_staged_frame_staged(form, kind):
    """frames_per_batch = 2 and one frame staged: nothing has been launched.  An asynchronous read with a NULL destination or a short pitch is
    refused with the code it always had, and the frame is STILL staged afterwards: the ctx's total of trace launches (bhray_get_level_grids)
    has not moved.  The next usable call launches the batch, gets ticket 0 and delivers."""
    rp = _open(form, frames_per_batch=2)
    P = _Probe(rp)
    rp.render()
    assert rp.level_grids(0)["total_launches"] == 0
    rowb = P.W * KINDS[kind]
    assert P.read_async(kind, None, rowb) == EXPECTED[form]["resolved"][f"{kind}.async.null"] == E_INVALID
    assert P.read_async(kind, P.pinned[kind].ptr, rowb - 1) == EXPECTED[form]["resolved"][f"{kind}.async.short"] == E_INVALID
    assert rp.level_grids(0)["total_launches"] == 0, "the refused read launched the staged batch"
    assert P.read_async(kind, P.pinned[kind].ptr, rowb) == OK and P.issued == 1
    assert rp.level_grids(0)["total_launches"] > 0
    P.close()
