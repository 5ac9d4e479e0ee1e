"""Host-side mirror of the reference's measurement-model interface `EMBA::LEGM`
(reference include/emba/model.h:72-133) on plain numpy arrays, calling the HIP library through the
C ABI of include/emba_hip.h.  Method names, argument meaning and error behaviour follow the reference:

    LEGM(camera_info, C_th, pano_width, pano_height)        model.h:76-77   -> LEGM(sensor_w, sensor_h, bearing_lut, ...)
    evaluateDataError(traj, Gx, Gy, events, eval_deriv, num_ev_map)  :83-84
    evaluateRegError / evaluateRobustDataCost                :87, :90       -> regCost / dataCost (scalar, on device)
    formNormalEq / formNormalEqIRLS                          :93-103
    applyL2Reg                                               :106-108

Differences forced by the boundary: the bearing-vector LUT is an input (the reference
builds it from ROS camera_info, event_pano_warper.cpp:27-41); the trajectory is passed as its control
quaternions + (t0_ns, dt_ns); events are registered once per window with set_events() because the per-pixel
event lists are pose-independent.  Invariant violations raise EmbaError (the reference aborts via glog CHECK).
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import EmbaCfg, EmbaError

_dp, _i32p, _u32p = _lib._dp, _lib._i32p, _lib._u32p
_u16p, _u8p, _i64p = _lib._u16p, _lib._u8p, _lib._i64p

COST_TYPES = {"quadratic": 0, "huber": 1, "cauchy": 2}
POISSON_BOUNDARIES = {"dirichlet": 0, "wrap": 1}      # EMBA_POISSON_DIRICHLET, EMBA_POISSON_WRAP_X


def poisson_boundary(boundary):
    """The boundary argument of reconstructIntensity / renderMapImages as the C ABI's integer."""
    if boundary not in POISSON_BOUNDARIES:
        raise ValueError(f"boundary must be 'dirichlet' or 'wrap', not {boundary!r}")
    return POISSON_BOUNDARIES[boundary]


def _p(a, ty):
    return None if a is None else a.ctypes.data_as(ty)


@dataclass
class LinearTrajectory:
    """The data `LinearTrajectory` hands to the hot path (reference include/utils/trajectory.h:109-190):
    control rotations as unit quaternions (x,y,z,w) and the spline timing of trajectory.cpp:59-64
    (t_beg_ns = int64(1e9*t_beg), dt_ns = int64(1e9*dt_knots))."""
    knots_xyzw: np.ndarray
    t0_ns: int
    dt_ns: int

    @classmethod
    def from_seconds(cls, t_beg, dt_knots, knots_xyzw):
        return cls(np.ascontiguousarray(knots_xyzw, dtype=np.float64).reshape(-1, 4), int(1e9 * t_beg), int(1e9 * dt_knots))

    def size(self):
        return self.knots_xyzw.shape[0]

    def evaluate(self, t_ns):
        """LinearTrajectory::evaluate (trajectory.cpp:122-147) on the host: the linear SO(3) spline at an integer-nanosecond time (so3.spline_evaluate)."""
        from . import so3
        return so3.spline_evaluate(self.knots_xyzw, self.t0_ns, self.dt_ns, t_ns)


@dataclass
class EventPacket:
    """std::vector<dvs_msgs::Event> (model.h:17) as a struct of arrays; ts as int64 nanoseconds."""
    x: np.ndarray
    y: np.ndarray
    polarity: np.ndarray
    t_ns: np.ndarray

    def size(self):
        return int(self.x.size)


@dataclass
class EventWindow:
    """event_subset_ = events_[beg, end) (emba.cpp:508-509) of the sequence LEGM.set_sequence left on the device: what set_events takes instead of an
    EventPacket in a sliding-window run (emba_set_events_seq)."""
    beg: int
    end: int

    def size(self):
        return int(self.end - self.beg)


class LEGM:
    def __init__(self, sensor_w, sensor_h, bearing_lut, C_th, pano_width, pano_height, device=0, stream=None):
        self._L = _lib.load()
        self._ctx = C.c_void_p()
        self.sensor_w, self.sensor_h = int(sensor_w), int(sensor_h)
        self.W, self.H = int(pano_width), int(pano_height)
        self.C_th = float(C_th)
        lut =np.ascontiguousarray(bearing_lut, dtype=np.float64).reshape(self.sensor_w * self.sensor_h, 3)
        cfg = EmbaCfg(self.sensor_w, self.sensor_h, self.W, self.H, _p(lut, _dp), float(C_th), 100, 10.0, int(device),
                      C.c_void_p(stream) if stream else None)
        st = self._L.emba_create(C.byref(cfg), C.byref(self._ctx))
        if st != _lib.OK:
            self._ctx = C.c_void_p()
            raise EmbaError(st, self._L.emba_last_error(None).decode())
        self.bearing_lut = lut                           # (host copy: the numpy forms of emba_amd.io that need the camera, e.g. cmax_objective)
        self.stream = int(stream) if stream else None   # the caller's HIP stream (None: the library made its own)
        self.n_events = 0
        self.K = 0
        self._P = 0
        self._keep = []  # arrays that must outlive an asynchronous launch

    # -- lifetime ------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._L.emba_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != _lib.OK:
            raise EmbaError(st, self._L.emba_last_error(self._ctx).decode())

    # -- events (once per window) --------------------------------------------------------------
    def set_events(self, events, halo=None):
        """events: EventPacket sorted by time, or an EventWindow of the resident sequence (set_sequence).  halo: optional (x, y, batch_t_ns) arrays
        (multi-GPU shards)."""
        if isinstance(events, EventWindow):
            if halo is not None:
                raise ValueError("a window of the resident sequence takes no halo")
            self._check(self._L.emba_set_events_seq(self._ctx, int(events.beg), int(events.end)))
            self.n_events = events.size()
            return
        x = np.ascontiguousarray(events.x, dtype=np.uint16)
        y = np.ascontiguousarray(events.y, dtype=np.uint16)
        pol = np.ascontiguousarray(events.polarity, dtype=np.uint8)
        t = np.ascontiguousarray(events.t_ns, dtype=np.int64)
        if not (x.size == y.size == pol.size == t.size):
            raise ValueError("event arrays differ in length")
        hx = hy = ht = None
        nh = 0
        if halo is not None and len(halo[0]):
            hx = np.ascontiguousarray(halo[0], dtype=np.uint16)
            hy = np.ascontiguousarray(halo[1], dtype=np.uint16)
            ht = np.ascontiguousarray(halo[2], dtype=np.int64)
            nh = hx.size
        self._check(self._L.emba_set_events(self._ctx, _p(x, _u16p), _p(y, _u16p), _p(pol, _u8p), _p(t, _i64p), x.size,
                                            _p(hx, _u16p), _p(hy, _u16p), _p(ht, _i64p), nh))
        self.n_events = x.size

    def set_events_dev(self, x_ptr, y_ptr, pol_ptr, t_ptr, n, halo=None):
        """The same with the arrays already in HBM: device pointers to uint16 x, uint16 y, uint8 polarity, int64 t_ns (n each);
        halo = (hx_ptr, hy_ptr, hbt_ptr, n_halo) or None.  Nothing of the per-window structure is built on the host."""
        hx = hy = ht = None
        nh = 0
        if halo is not None and halo[3]:
            hx, hy, ht, nh = C.c_void_p(halo[0]), C.c_void_p(halo[1]), C.c_void_p(halo[2]), int(halo[3])
        self._check(self._L.emba_set_events_dev(self._ctx, C.c_void_p(x_ptr), C.c_void_p(y_ptr), C.c_void_p(pol_ptr), C.c_void_p(t_ptr), int(n),
                                                hx, hy, ht, nh))
        self.n_events = int(n)

    # -- the whole sequence of a sliding-window run, resident on the device (emba.cpp:281-304, 473-510) ---------------------------
    def set_sequence(self, events, sampling_rate=1):
        """The whole recording to the device, once (emba_seq_upload): checked there and down-sampled as emba.cpp:281-304 does.  Returns the number of
        events kept (n // rate)."""
        x = np.ascontiguousarray(events.x, dtype=np.uint16)
        y = np.ascontiguousarray(events.y, dtype=np.uint16)
        pol = np.ascontiguousarray(events.polarity, dtype=np.uint8)
        t = np.ascontiguousarray(events.t_ns, dtype=np.int64)
        if not (x.size == y.size == pol.size == t.size):
            raise ValueError("event arrays differ in length")
        n = C.c_size_t(0)
        self._check(self._L.emba_seq_upload(self._ctx, _p(x, _u16p), _p(y, _u16p), _p(pol, _u8p), _p(t, _i64p), x.size, int(sampling_rate), C.byref(n)))
        return n.value

    def sequence_size(self):
        n = C.c_size_t(0)
        self._check(self._L.emba_seq_size(self._ctx, C.byref(n)))
        return n.value

    def sequence_window(self, t_beg_ns, t_end_ns):
        """EMBA::getEventSubset (emba.cpp:473-510) on the resident sequence: (beg, end).  Raises EmbaError where the window holds no events."""
        b, e = C.c_size_t(0), C.c_size_t(0)
        self._check(self._L.emba_seq_window(self._ctx, int(t_beg_ns), int(t_end_ns), C.byref(b), C.byref(e)))
        return b.value, e.value

    def set_events_seq_shard(self, win_beg, lo, hi):
        """This rank's part [lo, hi) of the window that begins at win_beg of the resident sequence (emba_set_events_seq_shard): the per-pixel halo of
        [win_beg, lo) is built on the device, nothing is sliced or sent from the host.  (lo - win_beg) % 100 == 0."""
        self._check(self._L.emba_set_events_seq_shard(self._ctx, int(win_beg), int(lo), int(hi)))
        self.n_events = int(hi) - int(lo)

    def sequence_halo(self, win_beg, lo):
        """The halo that registration builds, as (x, y, batch_t_ns) arrays (a download: tests, diagnostics) — what sharded.shard_events returns for the rank
        that begins at lo - win_beg of the slice [win_beg, ...)."""
        n = C.c_size_t(0)
        self._check(self._L.emba_seq_halo(self._ctx, int(win_beg), int(lo), None, None, None, 0, C.byref(n)))
        hx, hy, hbt = np.empty(n.value, np.uint16), np.empty(n.value, np.uint16), np.empty(n.value, np.int64)
        self._check(self._L.emba_seq_halo(self._ctx, int(win_beg), int(lo), _p(hx, _u16p), _p(hy, _u16p), _p(hbt, _i64p), n.value, C.byref(n)))
        return hx, hy, hbt

    def sequence_events(self, beg, end):
        """[beg, end) of the resident sequence as an EventPacket (a download: tests, diagnostics)."""
        n = int(end) - int(beg)
        x, y = np.empty(max(n, 0), np.uint16), np.empty(max(n, 0), np.uint16)
        pol, t = np.empty(max(n, 0), np.uint8), np.empty(max(n, 0), np.int64)
        self._check(self._L.emba_seq_get(self._ctx, int(beg), int(end), _p(x, _u16p), _p(y, _u16p), _p(pol, _u8p), _p(t, _i64p)))
        return EventPacket(x, y, pol, t)

    def filter_sequence(self, hot_sigma=0.0, refractory_ns=0, support_ns=0, sampling_rate=1):
        """Sensor noise out of the resident sequence, on the device (emba_seq_filter: hot pixels, refractory period, neighbour support — each event judged
        from the raw sequence; then the down-sampling of emba.cpp:281-304 over the survivors).  Returns stats = uint64[6]: events in, hot pixels, events
        failing hot / refractory / support, events kept.  io.filter_events is the same rule in numpy."""
        stats = np.zeros(6, np.uint64)
        self._check(self._L.emba_seq_filter(self._ctx, float(hot_sigma), int(refractory_ns), int(support_ns), int(sampling_rate),
                                            stats.ctypes.data_as(C.POINTER(C.c_uint64))))
        return stats

    def sequence_hot_pixels(self):
        """The hot pixels of the last filter_sequence: uint8[sensor_h * sensor_w], 1 = hot."""
        mask = np.zeros(self.sensor_w * self.sensor_h, np.uint8)
        self._check(self._L.emba_seq_hot_pixels(self._ctx, _p(mask, _u8p)))
        return mask

    def estimate_angular_velocity(self, slice_events, omega_max):
        """The angular velocity of every slice of slice_events events of the resident sequence by contrast maximisation, one launch (emba_seq_cmax; the
        rule: include/emba_hip.h).  Returns what io.estimate_angular_velocity returns, bit for bit: a dict of omega float64 [n_slices, 3], t_ref_ns int64
        [n_slices + 1] (empty where n_slices = 0), J0, J uint64 [n_slices], evals int32 [n_slices]."""
        u64p = C.POINTER(C.c_uint64)
        n = C.c_size_t(0)
        self._check(self._L.emba_seq_cmax(self._ctx, int(slice_events), float(omega_max), None, None, None, None, None, 0, C.byref(n)))
        ns = n.value
        out = dict(omega=np.zeros((ns, 3)), t_ref_ns=np.zeros(ns + 1 if ns else 0, np.int64), J0=np.zeros(ns, np.uint64), J=np.zeros(ns, np.uint64),
                   evals=np.zeros(ns, np.int32))
        if ns:
            self._check(self._L.emba_seq_cmax(self._ctx, int(slice_events), float(omega_max), _p(out["omega"], _dp), _p(out["t_ref_ns"], _i64p), _p(out["J0"], u64p),
                                              _p(out["J"], u64p), _p(out["evals"], _i32p), ns, C.byref(n)))
        return out

    def cmax_grid(self):
        """(shift, grid_w, grid_h) of the image of warped events on this sensor (io.cmax_grid)."""
        gw, gh, sh = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._check(self._L.emba_seq_cmax_objective(self._ctx, 0, 0, None, 0, None, None, C.byref(gw), C.byref(gh), C.byref(sh)))
        return sh.value, gw.value, gh.value

    def cmax_objective(self, omega, beg, end, want_iwe=True):
        """J of every candidate of omega [M, 3] over the events [beg, end) of the resident sequence, and their images of warped events
        (emba_seq_cmax_objective): (J uint64 [M], iwe uint32 [M, grid_h, grid_w] or None) — io.cmax_objective, bit for bit."""
        w = np.ascontiguousarray(omega, dtype=np.float64).reshape(-1, 3)
        _, gw, gh = self.cmax_grid()
        J = np.zeros(w.shape[0], np.uint64)
        iwe = np.zeros((w.shape[0], gh, gw), np.uint32) if want_iwe else None
        self._check(self._L.emba_seq_cmax_objective(self._ctx, int(beg), int(end), _p(w, _dp), w.shape[0], _p(J, C.POINTER(C.c_uint64)), _p(iwe, _u32p), None, None, None))
        return J, iwe

    def event_panorama(self, traj, beg=0, end=None, signed=False, want_image=True, want_pm=False, _chunk_events=None):
        """The panorama of warped events of [beg, end) of the resident sequence (end = None: its end) along the linear SO(3) spline traj, and its contrast
        (emba_seq_event_panorama; the rule: include/emba_hip.h): a dict of image int64 [pano_h, pano_w] (None with want_image=False), J = sum I^2, sum = sum I,
        nonzero = cells != 0, dropped = votes whose row lies outside the panorama (python ints) and pm float64 [nn, 2] (None without want_pm) —
        io.event_panorama given the same pm, bit for bit.  signed: events of polarity 0 vote negative.
        One library call counts fewer than 2^23 events exactly, so a longer range is cut here into chunks of whole batches (the batches, and so their
        midpoints and poses, are those of the uncut range), the chunks' int32 images are summed in int64, and J, sum and nonzero are then RECOMPUTED from
        that sum on the host (io.pano_contrast) — the chunks' own J do not add up to it; dropped and pm are the chunks' concatenated.  A range cut into
        chunks therefore always downloads the image, whatever want_image says about returning it."""
        from . import io as emba_io
        u64 = C.POINTER(C.c_uint64)
        knots = np.ascontiguousarray(traj.knots_xyzw, dtype=np.float64).reshape(-1, 4)
        end = self.sequence_size() if end is None else int(end)
        beg = int(beg)
        chunk = int(_chunk_events) if _chunk_events else (emba_io.PANO_MAX_EVENTS - 1) // emba_io.PANO_BATCH * emba_io.PANO_BATCH      # (private: the tests force small chunks)
        if chunk < emba_io.PANO_BATCH or chunk % emba_io.PANO_BATCH:
            raise ValueError("a chunk is a positive number of whole batches")
        nn = max(end - beg, 0) // emba_io.PANO_BATCH * emba_io.PANO_BATCH
        cuts = [(beg, end)] if nn <= chunk else [(b, min(b + chunk, beg + nn)) for b in range(beg, beg + nn, chunk)]
        single = len(cuts) == 1
        total = None if single else np.zeros((self.H, self.W), np.int64)
        pms, dropped, res = [], 0, None
        for b, e in cuts:
            m = max(e - b, 0) // emba_io.PANO_BATCH * emba_io.PANO_BATCH
            img = np.empty((self.H, self.W), np.int32) if (want_image or not single) else None
            pm = np.empty((m, 2)) if want_pm else None
            J, sm, nz, dr = C.c_uint64(0), C.c_int64(0), C.c_uint64(0), C.c_uint64(0)
            self._check(self._L.emba_seq_event_panorama(self._ctx, b, e, _p(knots, _dp), knots.shape[0], int(traj.t0_ns), int(traj.dt_ns), 1 if signed else 0,
                                                        _p(img, _i32p), C.byref(J), C.byref(sm), C.byref(nz), C.byref(dr), _p(pm, _dp)))
            dropped += dr.value
            if want_pm:
                pms.append(pm)
            if single:
                res = dict(image=None if img is None else img.astype(np.int64), J=J.value, sum=sm.value, nonzero=nz.value)
            else:
                total += img
        if not single:
            res = dict(emba_io.pano_contrast(total), image=total if want_image else None)
        res["dropped"] = dropped
        res["pm"] = (pms[0] if single else np.concatenate(pms)) if want_pm else None
        return res

    def render_views(self, frame_t_ns, knots, t0_ns, dt_ns, plane=None, boundary="dirichlet", fill=0.0, lo=None, hi=None, want_u8=False, want_pm=False):
        """What the camera would have seen at the times frame_t_ns [F] along the linear SO(3) spline (knots [K, 4], t0_ns, dt_ns): frames at sensor
        resolution sampled from `plane` [pano_h, pano_w], or, with plane=None, from the intensity panorama of the resident map under `boundary`
        (emba_render_views; the rule: include/emba_hip.h).  A dict of views float64 [F, sensor_h, sensor_w] (`fill` where a pixel looks past a pole row),
        outside int64 [F] (those pixels per frame), u8 uint8 [F, sensor_h, sensor_w] (None without want_u8) and pm float64 [F, sensor_h * sensor_w, 2] (None
        without want_pm) — io.render_views given the same pm, bit for bit.  The tone of u8 is sat(rint(255 / (hi - lo) (v - lo))); lo / hi default to the
        order statistics of normalizeRobust on the source plane (pct 0.1), so the tone is the panorama's own and constant across frames."""
        bc = poisson_boundary(boundary)
        knots = np.ascontiguousarray(knots, dtype=np.float64).reshape(-1, 4)
        ts = np.ascontiguousarray(frame_t_ns, dtype=np.int64).reshape(-1)
        F, S = ts.size, self.sensor_w * self.sensor_h
        if plane is not None:
            plane = np.ascontiguousarray(plane, dtype=np.float64)
            if plane.shape != (self.H, self.W):
                raise ValueError("plane must be pano_height x pano_width float64")
        if want_u8 and (lo is None or hi is None):
            rmin, rmax = self.normalizeRobust(self.reconstructIntensity(boundary=boundary) if plane is None else plane, with_range=True)[1]
            lo, hi = (rmin if lo is None else lo), (rmax if hi is None else hi)
        views = np.empty((F, self.sensor_h, self.sensor_w))
        u8 = np.empty((F, self.sensor_h, self.sensor_w), np.uint8) if want_u8 else None
        outside = np.zeros(F, np.uint64)
        pm = np.empty((F, S, 2)) if want_pm else None
        self._check(self._L.emba_render_views(self._ctx, _p(plane, _dp), bc, _p(ts, _i64p), F, _p(knots, _dp), knots.shape[0], int(t0_ns), int(dt_ns), float(fill),
                                              float(lo) if want_u8 else 0.0, float(hi) if want_u8 else 1.0, _p(views, _dp), _p(u8, _u8p),
                                              _p(outside, C.POINTER(C.c_uint64)), _p(pm, _dp)))
        return dict(views=views, outside=outside.astype(np.int64), u8=u8, pm=pm)

    def event_frames(self, beg, end, edge_t_ns, signed_polarity=True):
        """What the camera reported: the per-pixel event counts of the events [beg, end) of the resident sequence (end = None: its end) in the F frames whose
        edges are edge_t_ns [F + 1], strictly increasing (emba_seq_event_frames) — event k belongs to frame f when edge[f] <= t[k] < edge[f + 1], +1, or -1
        for polarity 0 with signed_polarity.  Every event counts, not whole batches of 100.  Returns (frames int32 [F, sensor_h, sensor_w], before, after):
        the events before edge[0] and at or after edge[F].  io.event_frames gives the same bits."""
        edges = np.ascontiguousarray(edge_t_ns, dtype=np.int64).reshape(-1)
        if edges.size < 1:
            raise ValueError("F frames have F + 1 edges: at least one")
        F = edges.size - 1
        end = self.sequence_size() if end is None else int(end)
        frames = np.zeros((F, self.sensor_h, self.sensor_w), np.int32)
        before, after = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.emba_seq_event_frames(self._ctx, int(beg), end, _p(edges, _i64p), F, 1 if signed_polarity else 0, _p(frames, _i32p), C.byref(before),
                                                  C.byref(after)))
        return frames, before.value, after.value

    def mosaic_frames(self, frames, frame_t_ns, traj, skip_zero=False, accumulate=False, want_pm=False):
        """Frames -> panorama (emba_mosaic_frames; the rule: include/emba_hip.h): the bytes frames [F, sensor_h, sensor_w] taken at the times frame_t_ns [F]
        are voted into the context's mosaic along traj (a LinearTrajectory) — every pixel bilinearly into four cells, its weight into sum_w, weight times
        byte into sum_v.  skip_zero: a byte of 0 casts no vote (the frames of render_views hold 0 outside the panorama).  accumulate: add to the sums that
        are there instead of starting from zero, so that frames can be streamed in pieces.  A dict of dropped (votes whose row lies outside the panorama),
        skipped (pixels skip_zero left out) and pm float64 [F, sensor_h * sensor_w, 2] (None without want_pm) — io.mosaic_votes given the same pm, the same
        integers."""
        ts = np.ascontiguousarray(frame_t_ns, dtype=np.int64).reshape(-1)
        F, S = ts.size, self.sensor_w * self.sensor_h
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.size != F * S:
            raise ValueError(f"frames must be {F} x sensor_height x sensor_width bytes")
        knots = np.ascontiguousarray(traj.knots_xyzw, dtype=np.float64).reshape(-1, 4)
        dropped, skipped = C.c_uint64(0), C.c_uint64(0)
        pm = np.empty((F, S, 2)) if want_pm else None
        self._check(self._L.emba_mosaic_frames(self._ctx, _p(frames, _u8p), _p(ts, _i64p), F, _p(knots, _dp), knots.shape[0], int(traj.t0_ns), int(traj.dt_ns),
                                               1 if skip_zero else 0, 1 if accumulate else 0, C.byref(dropped), C.byref(skipped), _p(pm, _dp)))
        return dict(dropped=dropped.value, skipped=skipped.value, pm=pm)

    def mosaic_frames_exposure(self, frames, frame_t_ns, traj, gain=None, bias=None, skip_zero=False, accumulate=False, want_pm=False):
        """mosaic_frames with a gain and a bias per frame (emba_mosaic_frames_exposure; the rule: include/emba_hip.h): frame f votes its compensated bytes
        clamp(rint(gain[f] v + bias[f]), 0, 255) in the place of v — io.mosaic_votes of io.exposure_bytes given the same pm, the same integers.  skip_zero
        tests the raw byte.  gain, bias: [F], a scalar for all frames, or None for 1 and 0 (which gives mosaic_frames' sums).  The dict of mosaic_frames."""
        ts = np.ascontiguousarray(frame_t_ns, dtype=np.int64).reshape(-1)
        F, S = ts.size, self.sensor_w * self.sensor_h
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.size != F * S:
            raise ValueError(f"frames must be {F} x sensor_height x sensor_width bytes")
        knots = np.ascontiguousarray(traj.knots_xyzw, dtype=np.float64).reshape(-1, 4)
        dropped, skipped = C.c_uint64(0), C.c_uint64(0)
        pm = np.empty((F, S, 2)) if want_pm else None
        a, b = self._exposure_args(gain, bias, F)
        self._check(self._L.emba_mosaic_frames_exposure(self._ctx, _p(frames, _u8p), _p(ts, _i64p), F, _p(a, _dp), _p(b, _dp), _p(knots, _dp), knots.shape[0],
                                                        int(traj.t0_ns), int(traj.dt_ns), 1 if skip_zero else 0, 1 if accumulate else 0, C.byref(dropped),
                                                        C.byref(skipped), _p(pm, _dp)))
        return dict(dropped=dropped.value, skipped=skipped.value, pm=pm)

    @staticmethod
    def _exposure_args(gain, bias, F):
        """gain, bias as contiguous float64 [F] (a scalar is broadcast; None is 1 or 0); what is in them is the entry point's to refuse."""
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(1.0 if gain is None else gain, dtype=np.float64), (F,)))
        b = np.ascontiguousarray(np.broadcast_to(np.asarray(0.0 if bias is None else bias, dtype=np.float64), (F,)))
        return a, b

    def mosaic(self, min_weight=256, fill=0.0):
        """The mosaic as it stands (emba_mosaic_get): a dict of sum_w, sum_v uint64 [pano_h, pano_w], covered bool (sum_w >= min_weight; 256 is one whole
        pixel's worth), mean float64 (sum_v / sum_w in byte units where covered, else `fill`) and n_covered — io.mosaic_mean of the sums, bit for bit."""
        shape = (self.H, self.W)
        sum_w, sum_v = np.empty(shape, np.uint64), np.empty(shape, np.uint64)
        mean, covered, n = np.empty(shape), np.empty(shape, np.uint8), C.c_uint64(0)
        u64p = C.POINTER(C.c_uint64)
        self._check(self._L.emba_mosaic_get(self._ctx, int(min_weight), float(fill), _p(sum_w, u64p), _p(sum_v, u64p), _p(mean, _dp), _p(covered, _u8p), C.byref(n)))
        return dict(sum_w=sum_w, sum_v=sum_v, mean=mean, covered=covered.astype(bool), n_covered=n.value)

    def mosaic_map(self, min_weight=256, lo=0.0, hi=1.0, eps=1.0 / 255.0, take_log=True, resident=False):
        """The log-intensity plane of the mosaic and the gradient map made from it (emba_mosaic_map): I = lo + mean (hi - lo) / 255, the inverse of
        render_views' tone; L = log(I + eps), or I itself without take_log (bytes that are log intensity already); Gx, Gy the backward differences of L
        between covered cells, 0 elsewhere — io.mosaic_log and io.gradient_from_plane.  resident: Gx, Gy also become the resident map, device to device, as
        upload_map of them would leave it.  A dict of L, Gx, Gy float64 [pano_h, pano_w]."""
        shape = (self.H, self.W)
        L, Gx, Gy = np.empty(shape), np.empty(shape), np.empty(shape)
        self._check(self._L.emba_mosaic_map(self._ctx, int(min_weight), float(lo), float(hi), float(eps), 1 if take_log else 0, _p(L, _dp), _p(Gx, _dp), _p(Gy, _dp),
                                            1 if resident else 0))
        return dict(L=L, Gx=Gx, Gy=Gy)

    def mosaic_clear(self):
        """Zero sums, nothing accumulated (emba_mosaic_clear)."""
        self._check(self._L.emba_mosaic_clear(self._ctx))

    def _align_args(self, frames, q_xyzw, plane, valid, use_mosaic):
        q = np.ascontiguousarray(q_xyzw, dtype=np.float64).reshape(-1, 4)
        F, S = q.shape[0], self.sensor_w * self.sensor_h
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.size != F * S:
            raise ValueError(f"frames must be {F} x sensor_height x sensor_width bytes")
        if plane is None and not use_mosaic:
            raise ValueError("a plane [pano_height, pano_width], or use_mosaic")
        if plane is not None:
            plane = np.ascontiguousarray(plane, dtype=np.float64)
            if plane.shape != (self.H, self.W):
                raise ValueError("plane must be pano_height x pano_width float64")
            if valid is not None:
                valid = np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.uint8)
                if valid.shape != (self.H, self.W):
                    raise ValueError("valid must be pano_height x pano_width")
        return frames, q, F, S, plane, (valid if plane is not None else None)

    def align_frames_eval(self, frames, q_xyzw, plane=None, valid=None, use_mosaic=False, min_weight=256, fill=0.0, lo=0.0, hi=255.0, skip_zero=False,
                          huber_k=0.0, want_pm=False, want_resid=False):
        """One evaluation of the photometric alignment of the bytes frames [F, sensor_h, sensor_w] at the rotations q_xyzw [F, 4] against `plane`
        [pano_h, pano_w] under the optional mask `valid`, or, with plane=None and use_mosaic, against the mosaic's mean under its covered cells
        (emba_frames_align_eval; the rule: include/emba_hip.h).  The frames' bytes mean I = lo + v (hi - lo) / 255 in the plane's units (the mosaic's mean
        is in byte units: lo = 0, hi = 255).  A dict of sums float64 [F, 10] (H's six entries 00 01 02 11 12 22, b's three, the cost), counts int64 [F, 4]
        (used, outside, masked, skipped), pm [F, S, 2] and resid [F, S] (None unless asked for) — io.align_terms and io.align_sums given the same pm."""
        frames, q, F, S, plane, valid = self._align_args(frames, q_xyzw, plane, valid, use_mosaic)
        sums, counts = np.zeros((F, 10)), np.zeros((F, 4), np.uint64)
        pm = np.empty((F, S, 2)) if want_pm else None
        resid = np.empty((F, S)) if want_resid else None
        self._check(self._L.emba_frames_align_eval(self._ctx, _p(frames, _u8p), F, _p(q, _dp), _p(plane, _dp), _p(valid, _u8p), 1 if use_mosaic else 0,
                                                   int(min_weight), float(fill), float(lo), float(hi), 1 if skip_zero else 0, float(huber_k), _p(sums, _dp),
                                                   _p(counts, C.POINTER(C.c_uint64)), _p(pm, _dp), _p(resid, _dp)))
        return dict(sums=sums, counts=counts.astype(np.int64), pm=pm, resid=resid)

    def align_frames(self, frames, q_xyzw, plane=None, valid=None, use_mosaic=False, min_weight=256, fill=0.0, lo=0.0, hi=255.0, skip_zero=False, **settings):
        """Poses from frames (emba_frames_align): every frame's own rotation refined by a 3-DoF Levenberg-Marquardt on its photometric error against the
        plane (arguments as align_frames_eval; settings: the members of io.ALIGN_DEFAULTS).  A dict of q [F, 4], sums [F, 10] and counts [F, 4] at q,
        status int32 [F] (io.ALIGN_CONVERGED / STALLED / ITERATIONS / DEGENERATE), iters [F] (trials evaluated), cost0 and n0 [F] (cost and used pixels
        at q_xyzw).  io.align_frames is the same loop in numpy."""
        from . import io as emba_io
        s = emba_io.align_settings(**settings)
        frames, q, F, S, plane, valid = self._align_args(frames, q_xyzw, plane, valid, use_mosaic)
        cs = _lib.EmbaAlignSettings(int(s["max_iters"]), int(s["min_pixels"]), float(s["lambda0"]), float(s["lambda_up"]), float(s["lambda_down"]),
                                    float(s["lambda_min"]), float(s["lambda_max"]), float(s["tol_rot"]), float(s["huber_k"]))
        q_out, sums, counts = q.copy(), np.zeros((F, 10)), np.zeros((F, 4), np.uint64)
        status, iters, cost0, n0 = np.zeros(F, np.int32), np.zeros(F, np.int32), np.zeros(F), np.zeros(F, np.uint64)
        u64p = C.POINTER(C.c_uint64)
        self._check(self._L.emba_frames_align(self._ctx, _p(frames, _u8p), F, _p(q, _dp), _p(plane, _dp), _p(valid, _u8p), 1 if use_mosaic else 0,
                                              int(min_weight), float(fill), float(lo), float(hi), 1 if skip_zero else 0, C.addressof(cs), _p(q_out, _dp),
                                              _p(sums, _dp), _p(counts, u64p), _p(status, _i32p), _p(iters, _i32p), _p(cost0, _dp), _p(n0, u64p)))
        return dict(q=q_out, sums=sums, counts=counts.astype(np.int64), status=status, iters=iters, cost0=cost0, n0=n0.astype(np.int64))

    def exposure_eval(self, frames, q_xyzw, gain=None, bias=None, plane=None, valid=None, use_mosaic=False, min_weight=256, fill=0.0, lo=0.0, hi=255.0,
                      skip_zero=False, huber_k=0.0, want_pm=False, want_resid=False):
        """align_frames_eval with a gain and a bias per frame (emba_frames_exposure_eval; the rule: include/emba_hip.h): the residual is
        val - (gain[f] I0 + bias[f]), the parameters are the rotation, the gain and the bias.  A dict of sums float64 [F, 21] (H's upper triangle over
        (delta, a, b) in row-major order, b's five, the cost), counts int64 [F, 4], pm and resid (None unless asked for) — io.exposure_terms and
        io.exposure_sums given the same pm."""
        frames, q, F, S, plane, valid = self._align_args(frames, q_xyzw, plane, valid, use_mosaic)
        a, b = self._exposure_args(gain, bias, F)
        sums, counts = np.zeros((F, 21)), np.zeros((F, 4), np.uint64)
        pm = np.empty((F, S, 2)) if want_pm else None
        resid = np.empty((F, S)) if want_resid else None
        self._check(self._L.emba_frames_exposure_eval(self._ctx, _p(frames, _u8p), F, _p(q, _dp), _p(a, _dp), _p(b, _dp), _p(plane, _dp), _p(valid, _u8p),
                                                      1 if use_mosaic else 0, int(min_weight), float(fill), float(lo), float(hi), 1 if skip_zero else 0,
                                                      float(huber_k), _p(sums, _dp), _p(counts, C.POINTER(C.c_uint64)), _p(pm, _dp), _p(resid, _dp)))
        return dict(sums=sums, counts=counts.astype(np.int64), pm=pm, resid=resid)

    def align_frames_exposure(self, frames, q_xyzw, gain=None, bias=None, estimate=3, plane=None, valid=None, use_mosaic=False, min_weight=256, fill=0.0,
                              lo=0.0, hi=255.0, skip_zero=False, gain_min=None, gain_max=None, **settings):
        """Poses and exposures from frames (emba_frames_exposure_align): align_frames with a gain and a bias per frame, estimated with the rotation where
        `estimate` (io.EXPOSURE_GAIN | io.EXPOSURE_BIAS) says so and kept otherwise; a trial whose estimated gain leaves [gain_min, gain_max]
        (io.EXPOSURE_BOUNDS) is rejected.  A dict of q [F, 4], gain, bias [F], sums [F, 21] and counts [F, 4] at them, status, iters, cost0, n0 [F].
        io.align_frames_exposure is the same loop in numpy."""
        from . import io as emba_io
        s = emba_io.align_settings(**settings)
        g_lo = float(emba_io.EXPOSURE_BOUNDS["gain_min"] if gain_min is None else gain_min)
        g_hi = float(emba_io.EXPOSURE_BOUNDS["gain_max"] if gain_max is None else gain_max)
        frames, q, F, S, plane, valid = self._align_args(frames, q_xyzw, plane, valid, use_mosaic)
        a, b = self._exposure_args(gain, bias, F)
        cs = _lib.EmbaExposureSettings(_lib.EmbaAlignSettings(int(s["max_iters"]), int(s["min_pixels"]), float(s["lambda0"]), float(s["lambda_up"]),
                                                              float(s["lambda_down"]), float(s["lambda_min"]), float(s["lambda_max"]), float(s["tol_rot"]),
                                                              float(s["huber_k"])), g_lo, g_hi)
        q_out, a_out, b_out, sums, counts = q.copy(), a.copy(), b.copy(), np.zeros((F, 21)), np.zeros((F, 4), np.uint64)
        status, iters, cost0, n0 = np.zeros(F, np.int32), np.zeros(F, np.int32), np.zeros(F), np.zeros(F, np.uint64)
        u64p = C.POINTER(C.c_uint64)
        self._check(self._L.emba_frames_exposure_align(self._ctx, _p(frames, _u8p), F, _p(q, _dp), _p(a, _dp), _p(b, _dp), int(estimate), _p(plane, _dp),
                                                       _p(valid, _u8p), 1 if use_mosaic else 0, int(min_weight), float(fill), float(lo), float(hi),
                                                       1 if skip_zero else 0, C.addressof(cs), _p(q_out, _dp), _p(a_out, _dp), _p(b_out, _dp), _p(sums, _dp),
                                                       _p(counts, u64p), _p(status, _i32p), _p(iters, _i32p), _p(cost0, _dp), _p(n0, u64p)))
        return dict(q=q_out, gain=a_out, bias=b_out, sums=sums, counts=counts.astype(np.int64), status=status, iters=iters, cost0=cost0, n0=n0.astype(np.int64))

    def track_frames(self, frames, frame_t_ns, q0=(0.0, 0.0, 0.0, 1.0), levels=(0,), batch=1, predict=True, skip_zero=False, min_weight=256, min_overlap=0.5,
                     want_pm=False, **settings):
        """Poses from the frames alone (emba_frames_track; the rule: include/emba_hip.h): frame 0 is put at q0, every later frame of frames
        [F, sensor_h, sensor_w] (taken at frame_t_ns [F], strictly increasing) is aligned to the mosaic of the frames tracked before it — level by level
        through `levels`, from a start predicted from the last two tracked frames — and then voted into it.  `batch` frames are aligned at once; settings:
        the members of io.ALIGN_DEFAULTS.  The mosaic the call leaves is the context's (mosaic, mosaic_map).  A dict of q [F, 4], status int32 [F]
        (io.TRACK_ANCHOR / TRACKED / LOST), iters [F, len(levels)], cost [F], counts [F, 4], overlap [F], tracked, lost, dropped, skipped and pm
        [F, S, 2] (None without want_pm; NaN for a lost frame).  io.track_frames is the same tracker in numpy."""
        from . import io as emba_io
        s = emba_io.align_settings(**settings)
        ts = np.ascontiguousarray(frame_t_ns, dtype=np.int64).reshape(-1)
        F, S = ts.size, self.sensor_w * self.sensor_h
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.size != F * S:
            raise ValueError(f"frames must be {F} x sensor_height x sensor_width bytes")
        levels = [int(l) for l in levels]
        if not 1 <= len(levels) <= 8:
            raise ValueError("a schedule names 1 ... 8 levels")
        q0 = np.ascontiguousarray(q0, dtype=np.float64).reshape(4)
        cs = _lib.EmbaTrackSettings(len(levels), (C.c_int32 * 8)(*levels), int(batch), 1 if predict else 0, 1 if skip_zero else 0, int(min_weight), float(min_overlap),
                                    _lib.EmbaAlignSettings(int(s["max_iters"]), int(s["min_pixels"]), float(s["lambda0"]), float(s["lambda_up"]), float(s["lambda_down"]),
                                                           float(s["lambda_min"]), float(s["lambda_max"]), float(s["tol_rot"]), float(s["huber_k"])))
        q, status, iters = np.zeros((F, 4)), np.zeros(F, np.int32), np.zeros((F, len(levels)), np.int32)
        cost, counts, overlap, stats = np.zeros(F), np.zeros((F, 4), np.uint64), np.zeros(F), np.zeros(4, np.uint64)
        pm = np.empty((F, S, 2)) if want_pm else None
        u64p = C.POINTER(C.c_uint64)
        self._check(self._L.emba_frames_track(self._ctx, _p(frames, _u8p), _p(ts, _i64p), F, _p(q0, _dp), C.addressof(cs), _p(q, _dp), _p(status, _i32p),
                                              _p(iters, _i32p), _p(cost, _dp), _p(counts, u64p), _p(overlap, _dp), _p(stats, u64p), _p(pm, _dp)))
        return dict(q=q, status=status, iters=iters, cost=cost, counts=counts.astype(np.int64), overlap=overlap, tracked=int(stats[0]), lost=int(stats[1]),
                    dropped=int(stats[2]), skipped=int(stats[3]), pm=pm)

    def track_eval(self, frames, q_xyzw, level=0, min_weight=256, skip_zero=False, huber_k=0.0, want_pm=False, want_resid=False):
        """One evaluation of the frames [F, sensor_h, sensor_w] at the rotations q_xyzw [F, 4] against the two integer sums of `level` as the last
        track_frames left them (emba_track_eval).  A dict as align_frames_eval's; pm is the level's — io.track_terms and io.align_sums given the same pm."""
        q = np.ascontiguousarray(q_xyzw, dtype=np.float64).reshape(-1, 4)
        F, S = q.shape[0], self.sensor_w * self.sensor_h
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.size != F * S:
            raise ValueError(f"frames must be {F} x sensor_height x sensor_width bytes")
        sums, counts = np.zeros((F, 10)), np.zeros((F, 4), np.uint64)
        pm = np.empty((F, S, 2)) if want_pm else None
        resid = np.empty((F, S)) if want_resid else None
        self._check(self._L.emba_track_eval(self._ctx, _p(frames, _u8p), F, _p(q, _dp), int(level), int(min_weight), 1 if skip_zero else 0, float(huber_k),
                                            _p(sums, _dp), _p(counts, C.POINTER(C.c_uint64)), _p(pm, _dp), _p(resid, _dp)))
        return dict(sums=sums, counts=counts.astype(np.int64), pm=pm, resid=resid)

    def track_level(self, level):
        """The two integer sums of a level as the last track_frames left them (emba_track_level_get): (sum_w, sum_v) uint64 [pano_h >> level, pano_w >> level]."""
        level = int(level)
        if not 0 <= level <= 7:
            raise ValueError("levels are 0 ... 7")
        shape = (self.H >> level, self.W >> level)
        sum_w, sum_v = np.zeros(shape, np.uint64), np.zeros(shape, np.uint64)
        u64p = C.POINTER(C.c_uint64)
        self._check(self._L.emba_track_level_get(self._ctx, level, _p(sum_w, u64p), _p(sum_v, u64p)))
        return sum_w, sum_v

    def track_frames_exposure(self, frames, frame_t_ns, q0=(0.0, 0.0, 0.0, 1.0), levels=(0,), batch=1, predict=True, skip_zero=False, min_weight=256,
                              min_overlap=0.5, estimate=3, gain_min=None, gain_max=None, want_pm=False, **settings):
        """track_frames for the frames of a camera with auto-exposure (emba_frames_track_exposure; the rule: include/emba_hip.h): every frame carries a gain
        and a bias beside its rotation, estimated with it at every level where `estimate` (io.EXPOSURE_GAIN | io.EXPOSURE_BIAS) says so, started at those of
        the last tracked frame, and a tracked frame votes its compensated bytes; a trial whose estimated gain leaves [gain_min, gain_max]
        (io.EXPOSURE_BOUNDS) is rejected.  estimate = 0 is track_frames.  track_frames' dict and gain, bias [F] (the anchor's: 1 and 0; a lost frame's: its
        start).  io.track_frames_exposure is the same tracker in numpy."""
        from . import io as emba_io
        s = emba_io.align_settings(**settings)
        g_lo = float(emba_io.EXPOSURE_BOUNDS["gain_min"] if gain_min is None else gain_min)
        g_hi = float(emba_io.EXPOSURE_BOUNDS["gain_max"] if gain_max is None else gain_max)
        ts = np.ascontiguousarray(frame_t_ns, dtype=np.int64).reshape(-1)
        F, S = ts.size, self.sensor_w * self.sensor_h
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.size != F * S:
            raise ValueError(f"frames must be {F} x sensor_height x sensor_width bytes")
        levels = [int(l) for l in levels]
        if not 1 <= len(levels) <= 8:
            raise ValueError("a schedule names 1 ... 8 levels")
        q0 = np.ascontiguousarray(q0, dtype=np.float64).reshape(4)
        ts_ = _lib.EmbaTrackSettings(len(levels), (C.c_int32 * 8)(*levels), int(batch), 1 if predict else 0, 1 if skip_zero else 0, int(min_weight), float(min_overlap),
                                     _lib.EmbaAlignSettings(int(s["max_iters"]), int(s["min_pixels"]), float(s["lambda0"]), float(s["lambda_up"]), float(s["lambda_down"]),
                                                            float(s["lambda_min"]), float(s["lambda_max"]), float(s["tol_rot"]), float(s["huber_k"])))
        cs = _lib.EmbaTrackExposureSettings(ts_, int(estimate), g_lo, g_hi)
        q, gain, bias, status, iters = np.zeros((F, 4)), np.zeros(F), np.zeros(F), np.zeros(F, np.int32), np.zeros((F, len(levels)), np.int32)
        cost, counts, overlap, stats = np.zeros(F), np.zeros((F, 4), np.uint64), np.zeros(F), np.zeros(4, np.uint64)
        pm = np.empty((F, S, 2)) if want_pm else None
        u64p = C.POINTER(C.c_uint64)
        self._check(self._L.emba_frames_track_exposure(self._ctx, _p(frames, _u8p), _p(ts, _i64p), F, _p(q0, _dp), C.addressof(cs), _p(q, _dp), _p(gain, _dp),
                                                       _p(bias, _dp), _p(status, _i32p), _p(iters, _i32p), _p(cost, _dp), _p(counts, u64p), _p(overlap, _dp),
                                                       _p(stats, u64p), _p(pm, _dp)))
        return dict(q=q, gain=gain, bias=bias, status=status, iters=iters, cost=cost, counts=counts.astype(np.int64), overlap=overlap, tracked=int(stats[0]),
                    lost=int(stats[1]), dropped=int(stats[2]), skipped=int(stats[3]), pm=pm)

    def track_exposure_eval(self, frames, q_xyzw, gain=None, bias=None, level=0, min_weight=256, skip_zero=False, huber_k=0.0, want_pm=False, want_resid=False):
        """track_eval with a gain and a bias per frame (emba_track_exposure_eval): the residual is val - (gain[f] v + bias[f]) against the two integer sums of
        `level` as the last tracker call left them.  A dict as exposure_eval's (sums [F, 21]); pm is the level's — io.track_exposure_terms and
        io.exposure_sums given the same pm."""
        q = np.ascontiguousarray(q_xyzw, dtype=np.float64).reshape(-1, 4)
        F, S = q.shape[0], self.sensor_w * self.sensor_h
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.size != F * S:
            raise ValueError(f"frames must be {F} x sensor_height x sensor_width bytes")
        a, b = self._exposure_args(gain, bias, F)
        sums, counts = np.zeros((F, 21)), np.zeros((F, 4), np.uint64)
        pm = np.empty((F, S, 2)) if want_pm else None
        resid = np.empty((F, S)) if want_resid else None
        self._check(self._L.emba_track_exposure_eval(self._ctx, _p(frames, _u8p), F, _p(q, _dp), _p(a, _dp), _p(b, _dp), int(level), int(min_weight),
                                                     1 if skip_zero else 0, float(huber_k), _p(sums, _dp), _p(counts, C.POINTER(C.c_uint64)), _p(pm, _dp),
                                                     _p(resid, _dp)))
        return dict(sums=sums, counts=counts.astype(np.int64), pm=pm, resid=resid)

    def refit_frames(self, frames, frame_t_ns, q, status, gain=None, bias=None, levels=(0,), batch=1, sweeps=1, alternate=True, recover=True, sweep_tol=0.0,
                     estimate=0, skip_zero=False, min_weight=256, min_overlap=0.5, gain_min=None, gain_max=None, want_pm=False, **settings):
        """A tracker's frames refitted against the mosaic of the other frames (emba_frames_refit; the rule: include/emba_hip.h): q [F, 4], status [F] and,
        from the tracker with exposure, gain and bias [F] (1 and 0 without) are what track_frames / track_frames_exposure returned.  The planes are built from
        every voting frame; then `sweeps` times every batch is taken out of them exactly, aligned to what is left — the frames before it and behind it — and
        voted back.  Anchors never move; with `recover` a lost frame starts between its voting neighbours and may become tracked; with `alternate` the odd
        sweeps run backwards; a sweep whose largest rotation change is below sweep_tol (rad) is the last.  sweeps = 0 stitches at the given rotations.  A
        dict of q, gain, bias, status, refit int32 [F] (io.REFIT_*), iters [F, len(levels)], cost, counts, overlap (the last sweep's), sweep
        [sweeps_done, 4] (moved, recovered, largest rotation change, sum of the last-level costs), sweeps_done, tracked, lost, dropped, skipped and pm
        [F, S, 2] (None without want_pm; NaN for a frame that does not vote).  io.refit_frames is the same rule in numpy."""
        from . import io as emba_io
        s = emba_io.align_settings(**settings)
        g_lo = float(emba_io.EXPOSURE_BOUNDS["gain_min"] if gain_min is None else gain_min)
        g_hi = float(emba_io.EXPOSURE_BOUNDS["gain_max"] if gain_max is None else gain_max)
        ts = np.ascontiguousarray(frame_t_ns, dtype=np.int64).reshape(-1)
        F, S = ts.size, self.sensor_w * self.sensor_h
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.size != F * S:
            raise ValueError(f"frames must be {F} x sensor_height x sensor_width bytes")
        levels = [int(l) for l in levels]
        if not 1 <= len(levels) <= 8:
            raise ValueError("a schedule names 1 ... 8 levels")
        q_in = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 4)
        st_in = np.ascontiguousarray(status, dtype=np.int32).reshape(-1)
        a_in, b_in = self._exposure_args(gain, bias, F)
        if q_in.shape[0] != F or st_in.size != F:
            raise ValueError(f"q must be [{F}, 4] and status [{F}]")
        sweeps = int(sweeps)
        ts_ = _lib.EmbaTrackSettings(len(levels), (C.c_int32 * 8)(*levels), int(batch), 0, 1 if skip_zero else 0, int(min_weight), float(min_overlap),
                                     _lib.EmbaAlignSettings(int(s["max_iters"]), int(s["min_pixels"]), float(s["lambda0"]), float(s["lambda_up"]), float(s["lambda_down"]),
                                                            float(s["lambda_min"]), float(s["lambda_max"]), float(s["tol_rot"]), float(s["huber_k"])))
        cs = _lib.EmbaRefitSettings(_lib.EmbaTrackExposureSettings(ts_, int(estimate), g_lo, g_hi), sweeps, 1 if alternate else 0, 1 if recover else 0, float(sweep_tol))
        q_out, a_out, b_out, st_out, refit = np.zeros((F, 4)), np.zeros(F), np.zeros(F), np.zeros(F, np.int32), np.zeros(F, np.int32)
        iters, cost, counts, overlap = np.zeros((F, len(levels)), np.int32), np.zeros(F), np.zeros((F, 4), np.uint64), np.zeros(F)
        sweep, done, stats = np.zeros((max(sweeps, 0), 4)), np.zeros(1, np.int32), np.zeros(4, np.uint64)
        pm = np.empty((F, S, 2)) if want_pm else None
        u64p = C.POINTER(C.c_uint64)
        self._check(self._L.emba_frames_refit(self._ctx, _p(frames, _u8p), _p(ts, _i64p), F, _p(q_in, _dp), _p(a_in, _dp), _p(b_in, _dp), _p(st_in, _i32p),
                                              C.addressof(cs), _p(q_out, _dp), _p(a_out, _dp), _p(b_out, _dp), _p(st_out, _i32p), _p(refit, _i32p), _p(iters, _i32p),
                                              _p(cost, _dp), _p(counts, u64p), _p(overlap, _dp), _p(sweep, _dp), _p(done, _i32p), _p(stats, u64p), _p(pm, _dp)))
        return dict(q=q_out, gain=a_out, bias=b_out, status=st_out, refit=refit, iters=iters, cost=cost, counts=counts.astype(np.int64), overlap=overlap,
                    sweep=sweep[:int(done[0])], sweeps_done=int(done[0]), tracked=int(stats[0]), lost=int(stats[1]), dropped=int(stats[2]), skipped=int(stats[3]),
                    pm=pm)

    def _pair_args(self, frames, pairs, Q_xyzw, gain, bias, calib):
        S = self.sensor_w * self.sensor_h
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.size % S:
            raise ValueError("frames must be F x sensor_height x sensor_width bytes")
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        P = pairs.shape[0]
        Q = np.ascontiguousarray(Q_xyzw, dtype=np.float64).reshape(-1, 4)
        if Q.shape[0] != P:
            raise ValueError(f"Q_xyzw must be [{P}, 4]")
        a = None if gain is None else np.ascontiguousarray(np.broadcast_to(np.asarray(gain, dtype=np.float64), (P,)))
        b = None if bias is None else np.ascontiguousarray(np.broadcast_to(np.asarray(bias, dtype=np.float64), (P,)))
        fu, fv, cu, cv = (float(calib[k]) for k in ("fu", "fv", "cu", "cv"))
        D = calib.get("D")
        D = None if D is None else np.ascontiguousarray(np.concatenate([np.asarray(D, dtype=np.float64).ravel(), np.zeros(5)])[:5])
        return frames, frames.size // S, S, pairs, P, Q, a, b, (fu, fv, cu, cv), D

    def pair_eval(self, frames, pairs, Q_xyzw, calib, gain=None, bias=None, skip_zero=False, huber_k=0.0, want_uv=False, want_resid=False):
        """One frame against another (emba_frames_pair_eval; the rule: include/emba_hip.h): for every pair (i, j) of `pairs` [P, 2] the normal equations of
        the photometric alignment of frame i's pixels to frame j's bytes at the relative rotation Q_xyzw [P, 4] and the relative exposure (gain, bias:
        [P], a scalar, or None for 1 and 0).  calib: a dict of fu, fv, cu, cv and D (five plumb_bob coefficients, or None).  A dict of sums [P, 10],
        counts int64 [P, 4], uv [P, S, 2] and resid [P, S] (None unless asked for) — io.pair_terms and io.pair_sums given the same uv."""
        frames, F, S, pairs, P, Q, a, b, k4, D = self._pair_args(frames, pairs, Q_xyzw, gain, bias, calib)
        sums, counts = np.zeros((P, 10)), np.zeros((P, 4), np.uint64)
        uv = np.empty((P, S, 2)) if want_uv else None
        resid = np.empty((P, S)) if want_resid else None
        self._check(self._L.emba_frames_pair_eval(self._ctx, _p(frames, _u8p), F, _p(pairs, _i32p), P, _p(Q, _dp), _p(a, _dp), _p(b, _dp), *k4, _p(D, _dp),
                                                  1 if skip_zero else 0, float(huber_k), _p(sums, _dp), _p(counts, C.POINTER(C.c_uint64)), _p(uv, _dp),
                                                  _p(resid, _dp)))
        return dict(sums=sums, counts=counts.astype(np.int64), uv=uv, resid=resid)

    def pair_align(self, frames, pairs, Q_xyzw, calib, gain=None, bias=None, skip_zero=False, **settings):
        """Relative rotations from pairs of frames (emba_frames_pair_align): every pair's Q refined by align_frames' loop on pair_eval's normal equations
        (arguments as pair_eval; settings: the members of io.ALIGN_DEFAULTS).  A dict of q [P, 4], sums [P, 10] and counts [P, 4] at q, status, iters,
        cost0, n0 [P] as align_frames', and info [P, 6]: the pair's information about its rotation (io.pair_information).  io.pair_align is the same
        loop in numpy."""
        from . import io as emba_io
        s = emba_io.align_settings(**settings)
        frames, F, S, pairs, P, Q, a, b, k4, D = self._pair_args(frames, pairs, Q_xyzw, gain, bias, calib)
        cs = _lib.EmbaAlignSettings(int(s["max_iters"]), int(s["min_pixels"]), float(s["lambda0"]), float(s["lambda_up"]), float(s["lambda_down"]),
                                    float(s["lambda_min"]), float(s["lambda_max"]), float(s["tol_rot"]), float(s["huber_k"]))
        q_out, sums, counts, info = Q.copy(), np.zeros((P, 10)), np.zeros((P, 4), np.uint64), np.zeros((P, 6))
        status, iters, cost0, n0 = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P), np.zeros(P, np.uint64)
        u64p = C.POINTER(C.c_uint64)
        self._check(self._L.emba_frames_pair_align(self._ctx, _p(frames, _u8p), F, _p(pairs, _i32p), P, _p(Q, _dp), _p(a, _dp), _p(b, _dp), *k4, _p(D, _dp),
                                                   1 if skip_zero else 0, C.addressof(cs), _p(q_out, _dp), _p(sums, _dp), _p(counts, u64p), _p(status, _i32p),
                                                   _p(iters, _i32p), _p(cost0, _dp), _p(n0, u64p), _p(info, _dp)))
        return dict(q=q_out, sums=sums, counts=counts.astype(np.int64), status=status, iters=iters, cost0=cost0, n0=n0.astype(np.int64), info=info)

    def pair_level_eval(self, frames, pairs, Q_xyzw, calib, level, gain=None, bias=None, skip_zero=False, huber_k=0.0, want_uv=False, want_resid=False,
                        want_level=False):
        """pair_eval on level `level` of the pyramid of the sensor frames, with the exposure's rows (emba_frames_pair_level_eval; the rule:
        include/emba_hip.h): a dict of sums [P, 21], counts int64 [P, 4], uv [P, S_l, 2], resid [P, S_l] and, with want_level, level_bytes uint8
        [F, sh_l, sw_l] and level_lut [S_l, 3] (None unless asked for) — io.pair_exposure_terms and io.pair_exposure_sums on io.pair_level_bytes,
        io.pair_level_lut and io.pair_level_calib, given the same uv."""
        frames, F, S, pairs, P, Q, a, b, k4, D = self._pair_args(frames, pairs, Q_xyzw, gain, bias, calib)
        level = int(level)
        wl, hl = (self.sensor_w >> level, self.sensor_h >> level) if 0 <= level <= 7 else (0, 0)
        Sl = wl * hl
        sums, counts = np.zeros((P, 21)), np.zeros((P, 4), np.uint64)
        uv = np.empty((P, Sl, 2)) if want_uv else None
        resid = np.empty((P, Sl)) if want_resid else None
        lb = np.zeros((F, hl, wl), np.uint8) if want_level else None
        ll = np.zeros((Sl, 3)) if want_level else None
        self._check(self._L.emba_frames_pair_level_eval(self._ctx, _p(frames, _u8p), F, _p(pairs, _i32p), P, _p(Q, _dp), _p(a, _dp), _p(b, _dp), *k4, _p(D, _dp),
                                                        1 if skip_zero else 0, float(huber_k), level, _p(sums, _dp), _p(counts, C.POINTER(C.c_uint64)),
                                                        _p(uv, _dp), _p(resid, _dp), _p(lb, _u8p), _p(ll, _dp)))
        return dict(sums=sums, counts=counts.astype(np.int64), uv=uv, resid=resid, level_bytes=lb, level_lut=ll)

    def pair_align_levels(self, frames, pairs, Q_xyzw, calib, levels=(0,), estimate=0, gain=None, bias=None, skip_zero=False, gain_min=None, gain_max=None,
                          **settings):
        """pair_align coarse to fine, with the pair's exposure estimated (emba_frames_pair_align_levels; the rule: include/emba_hip.h): every pair goes
        through the schedule `levels` (each 0 ... 7, level l the frames box-reduced by 2^l), from one level's accepted (Q, gain, bias) to the next, its
        relative gain and bias estimated where `estimate` (io.EXPOSURE_GAIN | io.EXPOSURE_BIAS) says so, within [gain_min, gain_max]
        (io.EXPOSURE_BOUNDS).  settings: the members of io.ALIGN_DEFAULTS.  A dict of q [P, 4], gain, bias [P], sums [P, 21] and counts [P, 4] of the last
        level run, status, iters (summed) [P], level_status, level_iters [P, n] (0: not run), cost0, n0 [P] of the first level, info [P, 6].
        io.pair_align_levels is the same schedule in numpy; levels = (0,) with estimate = 0 is pair_align bit for bit."""
        from . import io as emba_io
        s = emba_io.align_settings(**settings)
        g_lo = float(emba_io.EXPOSURE_BOUNDS["gain_min"] if gain_min is None else gain_min)
        g_hi = float(emba_io.EXPOSURE_BOUNDS["gain_max"] if gain_max is None else gain_max)
        frames, F, S, pairs, P, Q, a, b, k4, D = self._pair_args(frames, pairs, Q_xyzw, gain, bias, calib)
        lv = np.ascontiguousarray(levels, dtype=np.int32).reshape(-1)
        n = lv.size
        cs = _lib.EmbaExposureSettings(_lib.EmbaAlignSettings(int(s["max_iters"]), int(s["min_pixels"]), float(s["lambda0"]), float(s["lambda_up"]),
                                                              float(s["lambda_down"]), float(s["lambda_min"]), float(s["lambda_max"]), float(s["tol_rot"]),
                                                              float(s["huber_k"])), g_lo, g_hi)
        q_out, sums, counts, info = Q.copy(), np.zeros((P, 21)), np.zeros((P, 4), np.uint64), np.zeros((P, 6))
        a_out = np.ones(P) if a is None else a.copy()
        b_out = np.zeros(P) if b is None else b.copy()
        status, iters, cost0, n0 = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P), np.zeros(P, np.uint64)
        lst, lit = np.zeros((P, n), np.int32), np.zeros((P, n), np.int32)
        u64p = C.POINTER(C.c_uint64)
        self._check(self._L.emba_frames_pair_align_levels(self._ctx, _p(frames, _u8p), F, _p(pairs, _i32p), P, _p(Q, _dp), _p(a, _dp), _p(b, _dp), *k4, _p(D, _dp),
                                                          1 if skip_zero else 0, _p(lv, _i32p) if n else None, n, int(estimate), C.addressof(cs), _p(q_out, _dp),
                                                          _p(a_out, _dp), _p(b_out, _dp), _p(sums, _dp), _p(counts, u64p), _p(status, _i32p), _p(iters, _i32p),
                                                          _p(lst, _i32p), _p(lit, _i32p), _p(cost0, _dp), _p(n0, u64p), _p(info, _dp)))
        return dict(q=q_out, gain=a_out, bias=b_out, sums=sums, counts=counts.astype(np.int64), status=status, iters=iters, level_status=lst, level_iters=lit,
                    cost0=cost0, n0=n0.astype(np.int64), info=info)

    def _match_frames(self, frames):
        S = self.sensor_w * self.sensor_h
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.size % S:
            raise ValueError("frames must be F x sensor_height x sensor_width bytes")
        return frames, frames.size // S

    def match_eval(self, frames, pairs, level, rx, ry, skip_zero=False, n_min=1, want_sums=False):
        """The best shift of every pair of a list, by appearance (emba_frames_match_eval; the rule: include/emba_hip.h): level `level` of frames i and j
        compared under every shift |dx| <= rx, |dy| <= ry by the signed square of the zero-mean normalised correlation over the overlap, formed from six
        exact integer sums; a shift with fewer than n_min pixels or without variance is not scored.  A dict of score [P] (-2: no scored shift), shift int32
        [P, 2] (dx, dy), n int64 [P] and, with want_sums, sums uint64 [P, shifts, 6] (n, sum a, sum b, sum a^2, sum b^2, sum a b; shifts row-major, dy
        from -ry) — io.match_best and io.match_sums on io.pair_level_bytes, bit for bit."""
        frames, F = self._match_frames(frames)
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        P = pairs.shape[0]
        shifts = max((2 * int(rx) + 1) * (2 * int(ry) + 1), 0)
        score, shift, n = np.full(P, -2.0), np.zeros((P, 2), np.int32), np.zeros(P, np.uint64)
        sums = np.zeros((P, shifts, 6), np.uint64) if want_sums else None
        u64p = C.POINTER(C.c_uint64)
        self._check(self._L.emba_frames_match_eval(self._ctx, _p(frames, _u8p), F, _p(pairs, _i32p), P, int(level), int(rx), int(ry), 1 if skip_zero else 0,
                                                   int(n_min), _p(score, _dp), _p(shift, _i32p), _p(n, u64p), _p(sums, u64p)))
        return dict(score=score, shift=shift, n=n.astype(np.int64), sums=sums)

    def match_search(self, frames, status=None, level=0, rx=0, ry=0, min_gap=0, skip_zero=False, n_min=1, score_min=0.0, k=1):
        """Loop-closure pairs by appearance (emba_frames_match_search; the rule: include/emba_hip.h): every pair i < j of voting frames (status [F] of
        io.TRACK_*, None: all) with j - i > min_gap is scored as match_eval scores it, and per frame the k partners of greatest score >= score_min are kept,
        ties to the lower index.  A dict of partner int32 [F, k] (-1: none), score [F, k] (-2), shift int32 [F, k, 2] (from the lower index to the higher)
        and n int64 [F, k] — io.match_search, bit for bit; io.match_pairs makes the pairs of it."""
        frames, F = self._match_frames(frames)
        st = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(-1)
        if st is not None and st.size != F:
            raise ValueError(f"status must be [{F}]")
        K = max(int(k), 0)
        partner, score = np.full((F, K), -1, np.int32), np.full((F, K), -2.0)
        shift, n = np.zeros((F, K, 2), np.int32), np.zeros((F, K), np.uint64)
        self._check(self._L.emba_frames_match_search(self._ctx, _p(frames, _u8p), F, _p(st, _i32p), int(level), int(rx), int(ry), int(min_gap),
                                                     1 if skip_zero else 0, int(n_min), float(score_min), int(k), _p(partner, _i32p), _p(score, _dp),
                                                     _p(shift, _i32p), _p(n, C.POINTER(C.c_uint64))))
        return dict(partner=partner, score=score, shift=shift, n=n.astype(np.int64))

    @staticmethod
    def match_start(dx, dy, level, calib, sensor):
        """The rotation a matched pair starts from (emba_match_start; the rule: include/emba_hip.h): the shortest arc between the pinhole bearings of the
        two pixels the shift (dx, dy) of level `level` puts on the same place; calib: fu, fv, cu, cv (a lens is ignored); sensor: (sw, sh).  xyzw [4].  It
        needs no context and no device.  io.match_start is the same arithmetic in Python, bit for bit."""
        L = _lib.load()
        q = np.zeros(4)
        rc = L.emba_match_start(int(dx), int(dy), int(level), float(calib["fu"]), float(calib["fv"]), float(calib["cu"]), float(calib["cv"]), int(sensor[0]),
                                int(sensor[1]), _p(q, _dp))
        if rc != _lib.OK:
            raise _lib.EmbaError(rc, L.emba_last_error(None).decode())
        return q

    @staticmethod
    def rotation_graph_solve(q_xyzw, status, edges, Q_xyzw, info, **settings):
        """The rotation graph on the host (emba_rotation_graph_solve; the rule: include/emba_hip.h): q_xyzw [F, 4] with status [F] (io.TRACK_ANCHOR frames
        are held exactly), edges [E, 2] with their relative rotations Q_xyzw [E, 4] and information info [E, 6]; settings: the members of
        io.GRAPH_DEFAULTS.  A dict of q [F, 4], cost0, cost, iters, cg_iters, end (io.GRAPH_*).  It needs no context and no device.
        io.rotation_graph_solve is the same solve in numpy."""
        from . import io as emba_io
        s = emba_io.graph_settings(**settings)
        L = _lib.load()
        q = np.ascontiguousarray(q_xyzw, dtype=np.float64).reshape(-1, 4)
        st = np.ascontiguousarray(status, dtype=np.int32).reshape(-1)
        F = q.shape[0]
        if st.size != F:
            raise ValueError(f"status must be [{F}]")
        ed = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
        E = ed.shape[0]
        Qe = np.ascontiguousarray(Q_xyzw, dtype=np.float64).reshape(-1, 4)
        inf = np.ascontiguousarray(info, dtype=np.float64).reshape(-1, 6)
        if Qe.shape[0] != E or inf.shape[0] != E:
            raise ValueError(f"Q_xyzw must be [{E}, 4] and info [{E}, 6]")
        cs = _lib.EmbaGraphSettings(int(s["max_iters"]), int(s["cg_max_iters"]), float(s["lambda0"]), float(s["lambda_up"]), float(s["lambda_down"]),
                                    float(s["lambda_min"]), float(s["lambda_max"]), float(s["tol"]), float(s["cg_tol"]))
        q_out, cost, iters, end, at = q.copy(), np.zeros(2), np.zeros(2, np.int32), np.zeros(1, np.int32), C.c_size_t(0)
        rc = L.emba_rotation_graph_solve(_p(q, _dp), _p(st, _i32p), F, _p(ed, _i32p), _p(Qe, _dp), _p(inf, _dp), E, C.addressof(cs), _p(q_out, _dp),
                                         _p(cost, _dp), _p(iters, _i32p), _p(end, _i32p), C.byref(at))
        if rc != _lib.OK:
            err = _lib.EmbaError(rc, L.emba_last_error(None).decode())
            err.at = int(at.value)
            raise err
        return dict(q=q_out, cost0=float(cost[0]), cost=float(cost[1]), iters=int(iters[0]), cg_iters=int(iters[1]), end=int(end[0]))

    def simulate_events(self, step_t_ns, knots, t0_ns, dt_ns, plane=None, boundary="dirichlet", c_on=None, c_off=None, max_per_step=255, max_events=0):
        """A recording from a log-intensity plane and a trajectory, on the device (emba_simulate_events; the rule: include/emba_hip.h): the events of the
        F = len(step_t_ns) - 1 steps between the step times along the linear SO(3) spline (knots [K, 4], t0_ns, dt_ns), from the samples render_views gives
        at those times of `plane` [pano_h, pano_w], or, with plane=None, of the intensity panorama of the resident map under `boundary`.  c_on defaults to
        the model's C_th, c_off to c_on.  The recording stays on the device (simulated_events downloads it, sequence_from_simulation makes it the resident
        sequence).  Returns stats uint64 [4]: events, positive events, (pixel, step) pairs the cap cut short, (pixel, frame) pairs outside —
        io.simulate_events given the same samples, bit for bit.  More than max_events events (0: 2^32 - 2) raises EmbaError with status 6, and
        EmbaError.needed is the number that would have been needed."""
        bc = poisson_boundary(boundary)
        knots = np.ascontiguousarray(knots, dtype=np.float64).reshape(-1, 4)
        ts = np.ascontiguousarray(step_t_ns, dtype=np.int64).reshape(-1)
        if ts.size < 2:
            raise ValueError("F steps have F + 1 step times: at least two")
        if plane is not None:
            plane = np.ascontiguousarray(plane, dtype=np.float64)
            if plane.shape != (self.H, self.W):
                raise ValueError("plane must be pano_height x pano_width float64")
        c_on = float(self.C_th if c_on is None else c_on)
        c_off = c_on if c_off is None else float(c_off)
        stats = np.zeros(4, np.uint64)
        st = self._L.emba_simulate_events(self._ctx, _p(plane, _dp), bc, _p(ts, _i64p), ts.size - 1, _p(knots, _dp), knots.shape[0], int(t0_ns), int(dt_ns), c_on, c_off,
                                          int(max_per_step), int(max_events), stats.ctypes.data_as(C.POINTER(C.c_uint64)))
        if st != _lib.OK:
            err = EmbaError(st, self._L.emba_last_error(self._ctx).decode())
            err.needed = int(stats[0]) if st == _lib.ERR_CAPACITY else None
            raise err
        return stats

    def simulated_size(self):
        n = C.c_size_t(0)
        self._check(self._L.emba_sim_size(self._ctx, C.byref(n)))
        return n.value

    def simulated_events(self, beg=0, end=None):
        """[beg, end) of the simulated recording (end = None: its end) as an EventPacket (emba_sim_get): time order, ties by pixel index."""
        end = self.simulated_size() if end is None else int(end)
        n = max(end - int(beg), 0)
        x, y, pol, t = np.empty(n, np.uint16), np.empty(n, np.uint16), np.empty(n, np.uint8), np.empty(n, np.int64)
        self._check(self._L.emba_sim_get(self._ctx, int(beg), end, _p(x, _u16p), _p(y, _u16p), _p(pol, _u8p), _p(t, _i64p)))
        return EventPacket(x, y, pol, t)

    def sequence_from_simulation(self, sampling_rate=1):
        """The simulated recording becomes the resident sequence, device to device (emba_seq_from_sim): what set_sequence of simulated_events() with the same
        rate leaves.  Returns the number of events kept."""
        n = C.c_size_t(0)
        self._check(self._L.emba_seq_from_sim(self._ctx, int(sampling_rate), C.byref(n)))
        return n.value

    def contrast_gradient(self, traj, beg=0, end=None, signed=False, want_grad=True, want_image=False, want_pm=False, want_D=False, level=0, prior_weight=None):
        """The smooth (fp64, real bilinear weights) contrast J = sum I^2 of the panorama of warped events of [beg, end) of the resident sequence along the
        linear SO(3) spline traj, and its gradient with respect to the increments of io.incremental_update (emba_seq_contrast_gradient; the rule:
        include/emba_hip.h): a dict of J (float), grad float64 [3 K] (None with want_grad=False: the gradient pass is then not launched), dropped (int),
        image float64 [pano_h, pano_w] (None without want_image), pm float64 [nn, 2] (None without want_pm), D float64 [nn, 2, 6] and cp int32 [nn] (None
        without want_D).  io.contrast_gradient given the same pm, D and cp gives the same J, image and grad to the rounding of the sums' order.
        level > 0: the same on the grid of pano_w >> level by pano_h >> level cells (emba_seq_contrast_gradient_level) — image has that
        shape, pm and D stay the unscaled ones, and io.contrast_gradient on io.contrast_level(pm, D, pano_w, pano_h, level) is the numpy form.  level = 0
        goes through emba_seq_contrast_gradient as before there were levels.
        prior_weight = None: the calls above.  A number: the image starts as prior_weight times the level's prior (emba_seq_contrast_gradient_prior;
        DESIGN.md §15; contrast_prior_add / contrast_prior_set put one there) — io.contrast_gradient(..., prior=prior_weight * P) is the numpy form."""
        from . import io as emba_io
        knots = np.ascontiguousarray(traj.knots_xyzw, dtype=np.float64).reshape(-1, 4)
        end = self.sequence_size() if end is None else int(end)
        beg, level = int(beg), int(level)
        if level < 0:
            raise ValueError(f"level = {level}: levels are 0, 1, ...")
        nn = max(end - beg, 0) // emba_io.PANO_BATCH * emba_io.PANO_BATCH
        J, dr = C.c_double(0.0), C.c_uint64(0)
        grad = np.zeros(3 * knots.shape[0]) if want_grad else None
        img = np.zeros((self.H >> level, self.W >> level)) if want_image else None
        pm = np.zeros((nn, 2)) if want_pm else None
        D = np.zeros((nn, 2, 6)) if want_D else None
        cp = np.zeros(nn, np.int32) if want_D else None
        head = (self._ctx, beg, end, _p(knots, _dp), knots.shape[0], int(traj.t0_ns), int(traj.dt_ns), 1 if signed else 0)
        outs = (C.cast(C.byref(J), _dp), _p(grad, _dp), _p(img, _dp), C.byref(dr), _p(pm, _dp), _p(D, _dp), _p(cp, _i32p))
        if prior_weight is not None:
            self._check(self._L.emba_seq_contrast_gradient_prior(*head, level, float(prior_weight), *outs))
        elif level == 0:
            self._check(self._L.emba_seq_contrast_gradient(*head, *outs))
        else:
            self._check(self._L.emba_seq_contrast_gradient_level(*head, level, *outs))
        return dict(J=J.value, grad=grad, dropped=dr.value, image=img, pm=pm, D=D, cp=cp)

    def contrast_prior_add(self, traj, beg=0, end=None, levels=(0,), signed=False):
        """The votes of the used events of [beg, end) of the resident sequence along traj added to the priors of `levels`, one launch for all of them
        (emba_seq_contrast_prior_add): {"added": events used, "dropped": {level: votes whose row lies outside that level's grid}}."""
        from . import io as emba_io
        knots = np.ascontiguousarray(traj.knots_xyzw, dtype=np.float64).reshape(-1, 4)
        end = self.sequence_size() if end is None else int(end)
        levels = tuple(int(l) for l in levels)
        if any(not 0 <= l < 32 for l in levels):
            raise ValueError(f"levels {levels}: levels are 0 ... {emba_io.CONTRAST_MAX_LEVEL}")
        mask = 0
        for l in levels:
            mask |= 1 << l
        added = C.c_size_t(0)
        dropped = np.zeros(emba_io.CONTRAST_MAX_LEVEL + 1, np.uint64)
        self._check(self._L.emba_seq_contrast_prior_add(self._ctx, int(beg), end, _p(knots, _dp), knots.shape[0], int(traj.t0_ns), int(traj.dt_ns),
                                                        1 if signed else 0, mask, C.byref(added), _p(dropped, C.POINTER(C.c_uint64))))
        return dict(added=int(added.value), dropped={l: int(dropped[l]) for l in sorted(set(levels))})

    def contrast_prior_set(self, level, image):
        """The prior of `level` <- image [pano_h >> level, pano_w >> level]; None: no prior at that level (emba_seq_contrast_prior_set)."""
        level = int(level)
        if image is not None:
            image = np.ascontiguousarray(image, dtype=np.float64)
            if level < 0 or image.shape != (self.H >> level, self.W >> level):
                raise ValueError(f"the prior of level {level} has {self.H >> max(level, 0)} x {self.W >> max(level, 0)} cells, not {image.shape}")
        self._check(self._L.emba_seq_contrast_prior_set(self._ctx, level, _p(image, _dp)))

    def contrast_prior_get(self, level):
        """The prior of `level` as float64 [pano_h >> level, pano_w >> level], or None where there is none (emba_seq_contrast_prior_get)."""
        level = int(level)
        present = C.c_int32(0)
        self._check(self._L.emba_seq_contrast_prior_get(self._ctx, level, None, C.byref(present)))
        if not present.value:
            return None
        image = np.zeros((self.H >> level, self.W >> level))
        self._check(self._L.emba_seq_contrast_prior_get(self._ctx, level, _p(image, _dp), C.byref(present)))
        return image

    def contrast_prior_clear(self):
        """No prior at any level (emba_seq_contrast_prior_clear)."""
        self._check(self._L.emba_seq_contrast_prior_clear(self._ctx))

    def free_sequence(self):
        self._check(self._L.emba_seq_free(self._ctx))

    def median_blur_map(self):
        """emba.cpp:357-364 on the map resident on the device, both planes (emba_median_blur3_map)."""
        self._check(self._L.emba_median_blur3_map(self._ctx))

    def medianBlur3(self, plane):
        """The same 3x3 median (float32, replicated borders) of any 2-D float64 plane on the device: bit for bit io.median_blur3."""
        a = np.ascontiguousarray(plane, dtype=np.float64)
        if a.ndim != 2:
            raise ValueError("medianBlur3 takes a 2-D plane")
        out = np.empty_like(a)
        self._check(self._L.emba_median_blur3(self._ctx, _p(a, _dp), a.shape[0], a.shape[1], _p(out, _dp)))
        return out

    def setup_info(self):
        """Diagnostics of the once-per-window work (emba_last_setup_ms)."""
        a, b = C.c_double(0), C.c_double(0)
        t = C.c_int32(0)
        ne, nc = C.c_size_t(0), C.c_size_t(0)
        self._check(self._L.emba_last_setup_ms(self._ctx, C.byref(a), C.byref(b), C.byref(t), C.byref(ne), C.byref(nc)))
        pp, lf = C.c_double(0), C.c_double(0)
        self._check(self._L.emba_last_order_stats(self._ctx, C.byref(pp), C.byref(lf)))
        fi = C.c_double(0)
        self._check(self._L.emba_last_order_inlier_estimate(self._ctx, C.byref(fi)))
        g = [C.c_int32(0) for _ in range(5)]
        self._check(self._L.emba_last_tile_geometry(self._ctx, *[C.byref(v) for v in g]))
        return dict(set_events_ms=a.value, prepare_ms=b.value, tile_order=bool(t.value), entries=ne.value, chunks=nc.value,
                    events_per_pano_px=round(pp.value, 2), lead_in_frac=round(lf.value, 3), inlier_frac_predicted=round(fi.value, 3),
                    tile=dict(w=g[0].value, h=g[1].value, pitch_x=g[2].value, pitch_y=g[3].value, reserve=g[4].value) if t.value else None)

    def tile_drift(self):
        """(inliers of the last resolved evaluation outside their tile, times the window was re-binned): emba_last_tile_drift."""
        n, r = C.c_size_t(0), C.c_int32(0)
        self._check(self._L.emba_last_tile_drift(self._ctx, C.byref(n), C.byref(r)))
        return n.value, r.value

    def event_counts(self):
        a, b = C.c_size_t(0), C.c_size_t(0)
        self._check(self._L.emba_event_counts(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    # -- reference-shaped one-shot interface ---------------------------------------------------
    def evaluateDataError(self, traj, Gx, Gy, events=None, eval_deriv=True, num_ev_map=None):
        """model.cpp:72-258.  Returns ep (inlier residuals, reference order); fills num_ev_map (int32 H x W)."""
        if events is not None:
            self.set_events(events)
        if Gx is None and Gy is None:      # evaluate on the map already resident on the device (uploaded, updated or bound)
            pass
        else:
            Gx = np.ascontiguousarray(Gx, dtype=np.float64)
            Gy = np.ascontiguousarray(Gy, dtype=np.float64)
            if Gx.shape != (self.H, self.W) or Gy.shape != (self.H, self.W):
                raise ValueError("Gx/Gy must be pano_height x pano_width float64")
        knots = np.ascontiguousarray(traj.knots_xyzw, dtype=np.float64).reshape(-1, 4)
        self.K = knots.shape[0]
        ep = np.empty(max(self.n_events, 1), dtype=np.float64)
        n_inl = C.c_size_t(0)
        if num_ev_map is None:
            num_ev_map = np.empty((self.H, self.W), dtype=np.int32)
        assert num_ev_map.dtype == np.int32 and num_ev_map.flags.c_contiguous and num_ev_map.shape == (self.H, self.W)
        self._check(self._L.emba_eval_data_error(self._ctx, _p(knots, _dp), self.K, int(traj.t0_ns), int(traj.dt_ns), _p(Gx, _dp),
                                                 _p(Gy, _dp), 1 if eval_deriv else 0, _p(ep, _dp), C.byref(n_inl),
                                                 _p(num_ev_map, _i32p)))
        self.num_ev_map = num_ev_map
        return ep[:n_inl.value].copy()

    def dataCost(self, cost_type="quadratic", a=0.0):
        """0.5*ep.dot(ep) (solver.cpp:88) or evaluateRobustDataCost (model.cpp:279-314), reduced on the device."""
        v = C.c_double(0)
        self._check(self._L.emba_data_cost(self._ctx, COST_TYPES[cost_type], float(a), C.byref(v)))
        return v.value

    def costs(self, cost_type="quadratic", a=0.0, alpha=0.0):
        """(dataCost, regCost) with one host synchronisation: emba_costs."""
        d, r = C.c_double(0), C.c_double(0)
        self._check(self._L.emba_costs(self._ctx, COST_TYPES[cost_type], float(a), float(alpha), C.byref(d), C.byref(r)))
        return d.value, r.value

    def regCost(self, alpha):
        """alpha*0.5*|evaluateRegError|^2 (model.cpp:260-277, solver.cpp:90), reduced on the device."""
        v = C.c_double(0)
        self._check(self._L.emba_reg_cost(self._ctx, float(alpha), C.byref(v)))
        return v.value

    def _form(self, ep, thres, irls, a, alpha, dense_A12):
        ep_h = None if ep is None else np.ascontiguousarray(ep, dtype=np.float64)
        P = C.c_size_t(0)
        pl = C.c_size_t(0)
        self._check(self._L.emba_form_active(self._ctx, int(thres), C.byref(P), C.byref(pl)))
        self._P = P.value
        self._check(self._L.emba_form_accumulate(self._ctx, _p(ep_h, _dp), irls, float(a)))
        return self._finish(alpha, dense_A12)

    def _finish(self, alpha, dense_A12):
        P, dim = self._P, 3 * self.K
        A11 = np.zeros((dim, dim), order="F"); b1 = np.zeros(dim)
        active = np.zeros(max(P, 1), dtype=np.uint32)
        A22 = np.zeros((max(P, 1), 2, 2)); b2 = np.zeros(2 * max(P, 1))
        A12 = np.zeros((dim, 2 * P), order="F") if dense_A12 else None
        self._check(self._L.emba_form_finish(self._ctx, float(alpha), _p(A11, _dp), _p(b1, _dp), _p(active, _u32p), max(P, 1),
                                             _p(A22, _dp), _p(b2, _dp), _p(A12, _dp) if (dense_A12 and P) else None))
        return dict(A11=A11, b1=b1, active=active[:P].copy(), A22=A22[:P], b2=b2[:2 * P], A12=A12, P=P)

    def formNormalEq(self, ep, num_ctrl_poses, num_ev_map=None, thres_valid_pixel=5, dense_A12=False):
        """model.cpp:316-491.  num_ev_map is accepted for signature parity; the device-resident copy produced by the
        last evaluateDataError is what is used (they are the same object in the reference's call pattern, solver.cpp:114-126)."""
        if num_ctrl_poses != self.K:
            raise EmbaError(_lib.ERR_INVALID_ARG, "num_ctrl_poses differs from the trajectory used in evaluateDataError")
        return self._form(ep, thres_valid_pixel, 0, 0.0, 0.0, dense_A12)

    def formNormalEqIRLS(self, ep, num_ctrl_poses, num_ev_map=None, thres_valid_pixel=5, cost_type="huber", a=0.1,
                         dense_A12=False):
        """model.cpp:493-687."""
        if num_ctrl_poses != self.K:
            raise EmbaError(_lib.ERR_INVALID_ARG, "num_ctrl_poses differs from the trajectory used in evaluateDataError")
        return self._form(ep, thres_valid_pixel, COST_TYPES[cost_type], a, 0.0, dense_A12)

    def applyL2Reg(self, alpha, dense_A12=False):
        """model.cpp:689-719, applied to the device-resident pack; returns the updated blocks (call once per formNormalEq)."""
        return self._finish(alpha, dense_A12)

    keeps_equations_on_reject = True   # rejectMap / rejectTrial make the equations formed before the trial current again (second record set)
    async_phases = True            # eval_finish(sync=False) / form_active(thres, sync=False): the LM loop's only synchronisations are costs() and the solve
    supports_resident_x2 = True    # solveNormalEq[CG](..., resident_x2=True) returns x2 = None; updateMap(None, damping) applies the device copy

    def solveNormalEq(self, lam, fix_first_pose=False, resident_x2=False):
        """model.cpp:721-792 on the device-resident, L2-regularised normal equations (call after applyL2Reg, solver.cpp:130,190):
        returns (x1 [3K, zeros for a fixed first pose], x2 [2P]).  resident_x2: x2 stays on the device (returned as None) for the
        updateMap(None, ...) that follows — the reference hands it from the solver to updateMap and nowhere else (solver.cpp:193-239)."""
        self.last_counts()     # (P may have been left on the device by form_active(sync=False): the output buffer is sized from it)
        x1 = np.zeros(3 * self.K)
        x2 = None if resident_x2 else np.zeros(2 * max(self._P, 1))
        self._check(self._L.emba_solve_normal_eq(self._ctx, float(lam), 1 if fix_first_pose else 0, _p(x1, _dp), None if resident_x2 else _p(x2, _dp)))
        return x1, (None if resident_x2 else x2[:2 * self._P])

    def solveMapOnly(self, lam, resident_x2=False):
        """Mapping with known poses (emba_solve_map_only): x1 = 0 and, per active pixel, x2_i = (A22_i + lam diag A22_i)^-1 b2_i — the map block of the
        normal equations is block diagonal once the poses are held fixed, and well posed from an all-zero map.  Returns (zeros(3K), x2 [2P]);
        resident_x2 as in solveNormalEq: x2 is returned as None and updateMap(None, damping) applies the device copy."""
        self.last_counts()
        x2 = None if resident_x2 else np.zeros(2 * max(self._P, 1))
        self._check(self._L.emba_solve_map_only(self._ctx, float(lam), None if resident_x2 else _p(x2, _dp)))
        return np.zeros(3 * self.K), (None if resident_x2 else x2[:2 * self._P])

    def solvePosesOnly(self, lam, fix_first_pose=False):
        """Pose refinement against the map as it is (emba_solve_poses_only): (A11 + lam diag A11) x1 = b1.  Returns (x1 [3K], None): there is no map
        update, and updateMap(None, ...) raises until another solve leaves one."""
        x1 = np.zeros(3 * self.K)
        self._check(self._L.emba_solve_poses_only(self._ctx, float(lam), 1 if fix_first_pose else 0, _p(x1, _dp)))
        return x1, None

    def last_solve_info(self):
        """bit 0: a 2x2 block was not positive definite (the solve raised EMBA_ERR_NUMERIC); bit 1: a pivot of S vanished (zero update)."""
        v = C.c_int32(0)
        self._check(self._L.emba_last_solve_info(self._ctx, C.byref(v)))
        return v.value

    # -- sharded Schur solve: primitives around the caller's two collectives (emba_amd.sharded.ShardedLEGM.solveNormalEq) --------
    def solve_shard_size(self):
        n = C.c_size_t(0)
        self._check(self._L.emba_solve_shard_size(self._ctx, C.byref(n)))
        return n.value

    def solve_shard_count(self, n_ranks):
        counts = np.zeros(n_ranks, dtype=np.uint64)
        self._check(self._L.emba_solve_shard_count(self._ctx, int(n_ranks), counts.ctypes.data_as(_lib._szp)))
        return counts.astype(np.int64)

    def solve_shard_pack(self, n_ranks, send_ptr):
        self._check(self._L.emba_solve_shard_pack(self._ctx, int(n_ranks), C.c_void_p(send_ptr)))

    def solve_shard_cached(self, rank, n_ranks):
        """n_recv if this rank still holds the records it received for the current equations (a re-solve may skip the exchange), else None."""
        f, n = C.c_int32(0), C.c_size_t(0)
        self._check(self._L.emba_solve_shard_cached(self._ctx, int(rank), int(n_ranks), C.byref(f), C.byref(n)))
        return int(n.value) if f.value else None

    # -- sharded solveNormalEqCG: the per-rank steps (emba_cg_shard_*), driven by emba_amd.sharded.ShardedLEGM.solveNormalEqCG
    def cg_shard_size(self):
        n = C.c_size_t(0)
        self._check(self._L.emba_cg_shard_size(self._ctx, C.byref(n)))
        return n.value

    def cg_shard_begin(self, rank, n_ranks, recv_ptr, n_recv, lam, fix_first_pose, red_ptr):
        self._check(self._L.emba_cg_shard_begin(self._ctx, int(rank), int(n_ranks), C.c_void_p(recv_ptr), int(n_recv), float(lam), 1 if fix_first_pose else 0, C.c_void_p(red_ptr)))

    def cg_shard_apply(self, red_ptr):
        self._check(self._L.emba_cg_shard_apply(self._ctx, C.c_void_p(red_ptr)))

    def cg_shard_pt(self, red_ptr):
        v = C.c_double(0)
        self._check(self._L.emba_cg_shard_pt(self._ctx, C.c_void_p(red_ptr), C.byref(v)))
        return v.value

    def cg_shard_update(self, alpha, red_ptr):
        self._check(self._L.emba_cg_shard_update(self._ctx, float(alpha), C.c_void_p(red_ptr)))

    def cg_shard_direction(self, beta):
        self._check(self._L.emba_cg_shard_direction(self._ctx, float(beta)))

    def cg_shard_end(self, x2_full_ptr):
        x1 = np.zeros(3 * self.K)
        self._check(self._L.emba_cg_shard_end(self._ctx, _p(x1, _dp), C.c_void_p(x2_full_ptr)))
        return x1

    def solve_shard_partial(self, rank, n_ranks, recv_ptr, n_recv, lam, S_ptr):
        self._check(self._L.emba_solve_shard_partial(self._ctx, int(rank), int(n_ranks), C.c_void_p(recv_ptr), int(n_recv), float(lam), C.c_void_p(S_ptr)))

    def solve_shard_finish(self, rank, n_ranks, recv_ptr, n_recv, lam, fix_first_pose, S_ptr, x2_ptr):
        x1 = np.zeros(3 * self.K)
        self._check(self._L.emba_solve_shard_finish(self._ctx, int(rank), int(n_ranks), C.c_void_p(recv_ptr), int(n_recv), float(lam),
                                                    1 if fix_first_pose else 0, C.c_void_p(S_ptr), _p(x1, _dp), C.c_void_p(x2_ptr)))
        return x1

    def solveNormalEqCG(self, lam, fix_first_pose=False, max_iter=100, tol=1e-6, resident_x2=False):
        """model.cpp:794-840 (Eigen ConjugateGradient, 100 iterations, tolerance 1e-6) on the device: returns (x1, x2, iterations, error);
        resident_x2 as in solveNormalEq."""
        self.last_counts()
        x1 = np.zeros(3 * self.K)
        x2 = None if resident_x2 else np.zeros(2 * max(self._P, 1))
        it = C.c_int32(0); err = C.c_double(0)
        self._check(self._L.emba_solve_normal_eq_cg(self._ctx, float(lam), 1 if fix_first_pose else 0, int(max_iter), float(tol), _p(x1, _dp),
                                                    None if resident_x2 else _p(x2, _dp), C.byref(it), C.byref(err)))
        return x1, (None if resident_x2 else x2[:2 * self._P]), it.value, err.value

    def updateMap(self, x2, damping_factor):
        """model.cpp:863-903 on the device-resident map: builds the TRIAL map (active += damping*x2, all other pixels 0) that
        the following evaluateDataError(traj, None, None) uses; report the LM decision with acceptMap() / rejectMap().
        x2: a host array; None = the x2 the last solveNormalEq[CG] left on the device (resident_x2=True there saves the download
        too); or an int = device address of 2P doubles (a sharded host's all-reduced x2)."""
        if x2 is None:
            self._check(self._L.emba_update_map(self._ctx, None, float(damping_factor)))
        elif isinstance(x2, int):
            self._check(self._L.emba_update_map_dev(self._ctx, C.c_void_p(x2), float(damping_factor)))
        else:
            x2 = np.ascontiguousarray(x2, dtype=np.float64)
            self._check(self._L.emba_update_map(self._ctx, _p(x2, _dp), float(damping_factor)))

    def acceptMap(self):
        self._check(self._L.emba_map_accept(self._ctx))

    def rejectMap(self):
        self._check(self._L.emba_map_reject(self._ctx))

    def rejectTrial(self):
        """emba_trial_reject: the last evaluation was a rejected trial; the equations formed before it are current again."""
        self._check(self._L.emba_trial_reject(self._ctx))

    def downloadMap(self):
        Gx = np.empty((self.H, self.W)); Gy = np.empty((self.H, self.W))
        self._check(self._L.emba_download_map(self._ctx, _p(Gx, _dp), _p(Gy, _dp)))
        return Gx, Gy

    def set_cost(self, cost_type="quadratic", a=0.0):
        """Declare the robust cost of the formNormalEqIRLS calls to come, so that evaluations accumulate the IRLS-weighted
        per-pixel sums directly (speed only; see emba_set_cost)."""
        self._check(self._L.emba_set_cost(self._ctx, COST_TYPES[cost_type], float(a)))

    def reconstructIntensity(self, Gx=None, Gy=None, download=True, boundary="dirichlet"):
        """poisson_reconstruction::reconstructFromGradient (poisson_reconstruction.cpp:9-50; solver.cpp:417,471): the intensity
        panorama whose gradient is (Gx, Gy) — or the device-resident map when both are None.  boundary: "dirichlet", the reference's flat rectangle
        with intensity 0 all round, or "wrap": column W-1 is the neighbour of column 0, the rows beyond the poles stay 0 (include/emba_hip.h,
        EMBA_POISSON_WRAP_X) — no seam, and a map rolled by k columns gives the same panorama rolled."""
        bc = poisson_boundary(boundary)
        if (Gx is None) != (Gy is None):
            raise ValueError("pass both Gx and Gy, or neither")
        if Gx is not None:
            Gx = np.ascontiguousarray(Gx, dtype=np.float64); Gy = np.ascontiguousarray(Gy, dtype=np.float64)
            if Gx.shape != (self.H, self.W) or Gy.shape != (self.H, self.W):
                raise ValueError("Gx/Gy must be pano_height x pano_width float64")
        M = np.empty((self.H, self.W)) if download else None
        self._check(self._L.emba_reconstruct_intensity_bc(self._ctx, _p(Gx, _dp), _p(Gy, _dp), _p(M, _dp), bc))
        return M

    def renderMapImages(self, pct=0.1, poisson=True, boundary="dirichlet"):
        """The images EMBA::saveEvoData / saveOptData write (solver.cpp:370-479), rendered on the device from the map the next evaluation would
        use (the one downloadMap returns): {"Gx", "Gy": normalizeRobust(G, pct), "G_hsv": H x W x 3 RGB (hue = orientation, value = magnitude),
        "map_poisson": normalizeRobust(reconstructIntensity(boundary=boundary), pct) or None with poisson=False}, all uint8.  Synchronous: the
        images are in host memory when it returns."""
        bc = poisson_boundary(boundary)
        H, W = self.H, self.W
        gx, gy = np.empty((H, W), np.uint8), np.empty((H, W), np.uint8)
        rgb = np.empty((H, W, 3), np.uint8)
        mp = np.empty((H, W), np.uint8) if poisson else None
        self._check(self._L.emba_render_map_images_bc(self._ctx, float(pct), _p(gx, _u8p), _p(gy, _u8p), _p(rgb, _u8p), _p(mp, _u8p), bc))
        return {"Gx": gx, "Gy": gy, "G_hsv": rgb, "map_poisson": mp}

    def normalizeRobust(self, img, pct=0.1, with_range=False):
        """image_util::normalizeRobust (image_utils.cpp:14-38) of any float64 plane on the device: bit for bit io.normalize_robust.
        with_range=True also returns the order statistics (rmin, rmax)."""
        a = np.ascontiguousarray(img, dtype=np.float64)
        out = np.empty(a.shape, np.uint8)
        rmin, rmax = C.c_double(), C.c_double()
        self._check(self._L.emba_normalize_robust(self._ctx, _p(a, _dp), a.size, float(pct), _p(out, _u8p), C.byref(rmin), C.byref(rmax)))
        return (out, (rmin.value, rmax.value)) if with_range else out

    def A12_sparse(self):
        """Rank-1 factors of A12 (one per measurement candidate; pix == -1 marks outliers/inactive)."""
        _, M = self.event_counts()
        out = dict(cp_c=np.zeros(M, np.int32), cp_p=np.zeros(M, np.int32), pix=np.zeros(M, np.int32), w=np.zeros(M),
                   jc=np.zeros((M, 6)), jp=np.zeros((M, 6)), dp=np.zeros((M, 2)))
        self._check(self._L.emba_get_A12_sparse(self._ctx, _p(out["cp_c"], _i32p), _p(out["cp_p"], _i32p), _p(out["pix"], _i32p),
                                                _p(out["w"], _dp), _p(out["jc"], _dp), _p(out["jp"], _dp), _p(out["dp"], _dp)))
        return out

    def dump_state(self, fields=None):
        """Per-event State_LEGM (state.h:56-83) in original event order, for parity tests.  fields: subset of
        (pm, D, cp_idx, inlier_idx, pm_int, dp, Gpm, temp) — only those are produced (a 100 M-event pm dump is 1.6 GB, all of it 17 GB)."""
        n = self.n_events
        shapes = dict(pm=((n, 2), np.float64), D=((n, 2, 6), np.float64), cp_idx=((n,), np.int32), inlier_idx=((n,), np.int32),
                      pm_int=((n, 2), np.int32), dp=((n, 2), np.float64), Gpm=((n, 2), np.float64), temp=((n, 2), np.float64))
        want = list(shapes) if fields is None else list(fields)
        d = {k: np.zeros(shapes[k][0], shapes[k][1]) for k in want}
        g = lambda k, ty: _p(d[k], ty) if k in d else None
        self._check(self._L.emba_dump_state(self._ctx, g("pm", _dp), g("D", _dp), g("cp_idx", _i32p), g("inlier_idx", _i32p),
                                            g("pm_int", _i32p), g("dp", _dp), g("Gpm", _dp), g("temp", _dp)))
        return d

    def dump_segments(self):
        """The segment records {p0, delta, r1, k, r2} the last evaluation left on the device, (K - 1) x 12 (none with the per-batch pose table), for parity tests."""
        n = C.c_size_t()
        self._check(self._L.emba_dump_segments(self._ctx, None, 0, C.byref(n)))
        seg = np.zeros((n.value, 12))
        if n.value:
            self._check(self._L.emba_dump_segments(self._ctx, _p(seg, _dp), n.value, None))
        return seg

    # -- phase-level, HBM-resident interface (bench.py, sharded host) -------------------------------
    def upload_map(self, Gx, Gy):
        Gx = np.ascontiguousarray(Gx, dtype=np.float64); Gy = np.ascontiguousarray(Gy, dtype=np.float64)
        self._check(self._L.emba_upload_map(self._ctx, _p(Gx, _dp), _p(Gy, _dp)))
        self._check(self._L.emba_sync(self._ctx))

    def bind_map_dev(self, gx_ptr, gy_ptr):
        self._check(self._L.emba_bind_map_dev(self._ctx, C.c_void_p(gx_ptr), C.c_void_p(gy_ptr)))

    def bind_exchange_buffers(self, count_ptr, pack_ptr, pack_cap):
        self._check(self._L.emba_bind_exchange_buffers(self._ctx, C.c_void_p(count_ptr) if count_ptr else None,
                                                       C.c_void_p(pack_ptr) if pack_ptr else None, int(pack_cap)))

    def count_map_ready(self):
        """Make the device count map hold the counts of the last evaluation (call before reading / all-reducing a bound map)."""
        self._check(self._L.emba_count_map_ready(self._ctx))

    def count_compress(self, u8_ptr, cap):
        self._check(self._L.emba_count_compress(self._ctx, C.c_void_p(u8_ptr), int(cap)))

    def count_expand(self, u8_ptr):
        self._check(self._L.emba_count_expand(self._ctx, C.c_void_p(u8_ptr)))

    def eval_launch(self, traj):
        knots = np.ascontiguousarray(traj.knots_xyzw, dtype=np.float64).reshape(-1, 4)
        self.K = knots.shape[0]
        self._keep = [knots]
        self._check(self._L.emba_eval_launch(self._ctx, _p(knots, _dp), self.K, int(traj.t0_ns), int(traj.dt_ns)))

    def eval_finish(self, want_ep=False, want_map=False, sync=True):
        if not sync and not want_ep and not want_map:      # enqueue only; counts via last_counts() after a sync point
            self._check(self._L.emba_eval_finish(self._ctx, None, None, None))
            return None, None, None
        n_inl = C.c_size_t(0)
        ep = np.empty(max(self.n_events, 1)) if want_ep else None
        nem = np.empty((self.H, self.W), dtype=np.int32) if want_map else None
        self._check(self._L.emba_eval_finish(self._ctx, _p(ep, _dp), C.byref(n_inl), _p(nem, _i32p)))
        return n_inl.value, (ep[:n_inl.value] if want_ep else None), nem

    def form_active(self, thres, sync=True):
        if not sync:
            self._check(self._L.emba_form_active(self._ctx, int(thres), None, None))
            return None, None
        P, pl = C.c_size_t(0), C.c_size_t(0)
        self._check(self._L.emba_form_active(self._ctx, int(thres), C.byref(P), C.byref(pl)))
        self._P = P.value
        return P.value, pl.value

    def step_form_active(self, thres, global_u8_ptr=None):
        """F1 of a resident step on a rank of a sharded window (emba_step_form_active): activity from the all-reduced saturated byte counts."""
        self._check(self._L.emba_step_form_active(self._ctx, int(thres), C.c_void_p(global_u8_ptr) if global_u8_ptr else None))

    def form_accumulate(self, cost_type="quadratic", a=0.0):
        self._check(self._L.emba_form_accumulate(self._ctx, None, COST_TYPES[cost_type], float(a)))

    def form_finish(self, alpha, download=False, dense_A12=False):
        if download:
            self.last_counts()
            return self._finish(alpha, dense_A12)
        self._check(self._L.emba_form_finish(self._ctx, float(alpha), None, None, None, 0, None, None, None))
        return None

    def last_counts(self):
        a, b = C.c_size_t(0), C.c_size_t(0)
        self._check(self._L.emba_last_counts(self._ctx, C.byref(a), C.byref(b)))
        self._P = b.value
        return a.value, b.value

    def step(self, traj, thres_valid_pixel, alpha, cost_type="quadratic", a=0.0):
        """One whole resident step (evaluateDataError + formNormalEq[IRLS] + applyL2Reg) in a single library call."""
        if getattr(self, "_step_traj", None) is not traj:       # cache the contiguous knot array of this trajectory object
            self._step_knots = np.ascontiguousarray(traj.knots_xyzw, dtype=np.float64).reshape(-1, 4)
            self._step_traj = traj
        knots = self._step_knots
        self.K = knots.shape[0]
        a_, b_ = C.c_size_t(0), C.c_size_t(0)
        self._check(self._L.emba_step(self._ctx, _p(knots, _dp), self.K, int(traj.t0_ns), int(traj.dt_ns), int(thres_valid_pixel),
                                      COST_TYPES[cost_type], float(a), float(alpha), C.byref(a_), C.byref(b_)))
        self._P = b_.value
        return a_.value, b_.value

    def get_ep(self):
        """The last evaluation's residual vector in the reference's order, as the resident step left it on the device (or compacted now)."""
        n = C.c_size_t(0)
        ep = np.empty(max(int(self.n_events), 1), dtype=np.float64)
        self._check(self._L.emba_get_ep(self._ctx, _p(ep, _dp), ep.size, C.byref(n)))
        return ep[: n.value].copy()

    def set_option(self, name, value):
        """Tuning / A-B switch by name (include/emba_hip.h: emba_set_option); results do not depend on any of them."""
        self._check(self._L.emba_set_option(self._ctx, name.encode(), int(value)))

    def get_option(self, name):
        v = C.c_int32(0)
        self._check(self._L.emba_get_option(self._ctx, name.encode(), C.byref(v)))
        return v.value

    def compact_ep(self):
        """Enqueue the residual compaction into the reference-order `ep` vector on the device (emba_compact_ep)."""
        self._check(self._L.emba_compact_ep(self._ctx))

    def sync(self):
        self._check(self._L.emba_sync(self._ctx))

    def timer_start(self, slot=0):
        self._check(self._L.emba_timer_start(self._ctx, slot))

    def timer_stop(self, slot=0):
        self._check(self._L.emba_timer_stop(self._ctx, slot))

    def timer_ms(self, slot=0):
        ms = C.c_float(0)
        self._check(self._L.emba_timer_elapsed_ms(self._ctx, slot, C.byref(ms)))
        return ms.value

    def enable_kernel_timing(self, on=True, slot=0):
        """on: the next step's warp / Gram kernels are bracketed by HIP events in `slot` (< 16); read them with last_kernel_ms() at once or with
        kernel_ms_slot(slot) after the loop (no host wait inside it)."""
        self._check(self._L.emba_enable_kernel_timing(self._ctx, (1 + int(slot)) if on else 0))

    def kernel_ms_slot(self, slot):
        a, b = C.c_float(0), C.c_float(0)
        self._check(self._L.emba_kernel_ms_slot(self._ctx, int(slot), C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_kernel_ms(self):
        a, b = C.c_float(0), C.c_float(0)
        self._check(self._L.emba_last_kernel_ms(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def kernel_timing_all(self, on=True):
        """Sampled steps also record an event in front of their first launch: kernel_ms_all(slot) then returns the four intervals that tile the
        step's device time (prep || pose || texel, warp, post-warp launch A, Gram)."""
        self._check(self._L.emba_kernel_timing_all(self._ctx, 1 if on else 0))

    def kernel_ms_all(self, slot):
        v = (C.c_float * 4)()
        self._check(self._L.emba_kernel_ms_all(self._ctx, int(slot), v))
        return [float(x) for x in v]

    def bracket_overhead_us(self, reps=50):
        """Mean HIP-event interval around an EMPTY kernel queued behind running work: what a bracket reads for a kernel of zero length."""
        us = C.c_float(0)
        self._check(self._L.emba_bracket_overhead_us(self._ctx, int(reps), C.byref(us)))
        return us.value

    def clock_probe(self):
        """Device clock attributes and the shader clock measured by a probe kernel while the whole chip is busy (emba_clock_probe)."""
        sclk, us, ratio = C.c_double(0), C.c_double(0), C.c_double(0)
        cr, mr, wr = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._check(self._L.emba_clock_probe(self._ctx, C.byref(sclk), C.byref(us), C.byref(ratio), C.byref(cr), C.byref(mr), C.byref(wr)))
        return {"sclk_mhz_measured": sclk.value, "probe_us": us.value, "cycles_per_dependent_add": ratio.value,
                "attr_clock_rate_khz": cr.value, "attr_mem_clock_rate_khz": mr.value, "attr_wall_clock_rate_khz": wr.value}

    def pci_bus_id(self):
        buf = C.create_string_buffer(32)
        self._check(self._L.emba_device_pci_bus_id(self._ctx, buf, 32))
        return buf.value.decode()
