"""Data formats and trajectory plumbing on either side of the hot path, without ROS.  Mirrors:

  load_map / save_map            EMBA::loadMap                       src/emba/emba.cpp:535-578   (Gx.bin / Gy.bin, raw f64 row-major,
                                                                                                  H = sqrt(n/2), W = 2H)
  load_poses                     PoseManager::loadPoses              src/utils/pose_manager.cpp:41-80  ("ts tx ty tz qx qy qz qw" per line)
  pose_at                        PoseManager::getPoseAt              :82-108                      (geodesic interpolation)
  write_trajectory               LinearTrajectory::write             src/utils/trajectory.cpp:98-114
  fit_ctrl_poses                 LinearTrajectory::fitCtrlPoses      :149-229                     (tangent-space least squares)
  generate_ctrl_poses_long       LinearTrajectory::generateCtrlPosesLong  :258-294
  incremental_update             LinearTrajectory::incrementalUpdate :296-304                     (left perturbation exp(x)*knot)
  bearing_lut_from_calibration   EventWarper::precomputeBearingVectors src/utils/event_pano_warper.cpp:27-41 (image_geometry rectifyPoint +
                                                                      projectPixelTo3dRay for a monocular plumb_bob camera)
  normalize_robust / save_pgm    image_util::normalizeRobust          src/utils/image_utils.cpp:13-38   (8-bit display images of maps and of the
                                                                      Poisson-reconstructed panorama, solver.cpp:417-425; PGM instead of PNG)
  save_png                       cv::imwrite of an 8-bit image         solver.cpp:381-479 (record_data's map images; grey or RGB, standard-library zlib)
  ros_time_ns                    ros::Time(double) / ros::Duration(double) -> toNSec()  (rostime)
  downsample_events              the event down-sampling of EMBA::EMBA   src/emba/emba.cpp:281-304
  event_window                   EMBA::getEventSubset                 src/emba/emba.cpp:473-510
  median_blur3                   convertTo(CV_32F) + cv::medianBlur(3) + convertTo(CV_64F) of the initial map   src/emba/emba.cpp:357-364
  save_events / load_events      a flat .npz replacing the rosbag of src/utils/rosbag_loading.cpp (x, y u16; polarity u8; t_ns i64, sorted)

Host-side, O(K) or file-sized work; the per-event path is emba_amd.LEGM.
"""
import os

import numpy as np

from . import so3
from .legm import EventPacket, LinearTrajectory


# ---- panoramic gradient map ------------------------------------------------------------------------------------------
def load_map(map_dir):
    gx = np.fromfile(os.path.join(map_dir, "Gx.bin"), dtype="<f8")
    gy = np.fromfile(os.path.join(map_dir, "Gy.bin"), dtype="<f8")
    if gx.size != gy.size:
        raise ValueError("Gx.bin and Gy.bin differ in size")                    # CHECK_EQ, emba.cpp:566
    H = int(np.sqrt(gx.size / 2))                                               # emba.cpp:552
    W = 2 * H
    if H * W != gx.size:
        raise ValueError(f"{gx.size} doubles is not an H x 2H panorama")
    return gx.reshape(H, W).copy(), gy.reshape(H, W).copy()


def save_map(map_dir, Gx, Gy):
    os.makedirs(map_dir, exist_ok=True)
    np.ascontiguousarray(Gx, dtype="<f8").tofile(os.path.join(map_dir, "Gx.bin"))
    np.ascontiguousarray(Gy, dtype="<f8").tofile(os.path.join(map_dir, "Gy.bin"))


# ---- poses --------------------------------------------------------------------------------------------------------------
def load_poses(path, time_offset=0.0):
    """Returns (t [n] seconds ascending, q [n,4] xyzw unit); lines that do not parse as 8 numbers are skipped like the reference's `if (ss >> ...)`."""
    ts, qs = [], []
    with open(path) as f:
        for line in f:
            parts = line.split()
            if len(parts) < 8:
                continue
            try:
                v = [float(x) for x in parts[:8]]
            except ValueError:
                continue
            ts.append(v[0] + time_offset)
            qs.append(so3.normalize(v[4:8]))                                   # Sophus::SO3d(q) normalises
    order = np.argsort(np.array(ts), kind="stable")                            # std::map<ros::Time, SO3d>
    return np.array(ts)[order], np.array(qs).reshape(-1, 4)[order]


def pose_at(t, qs, t_query):
    """PoseManager::getPoseAt: clamp outside, R1 * exp(s * log(R1^-1 R2)) inside."""
    i2 = int(np.searchsorted(t, t_query, side="right"))                        # upper_bound
    if i2 == 0:
        return qs[0]
    if i2 == len(t):
        return qs[-1]
    q1, q2 = qs[i2 - 1], qs[i2]
    s = (t_query - t[i2 - 1]) / (t[i2] - t[i2 - 1])
    return so3.mul(q1, so3.exp(s * so3.log(so3.mul(so3.inverse(q1), q2))))


def write_trajectory(path, traj, time_offset=0.0):
    """`t 0 0 0 qx qy qz qw` per control pose; numbers as an std::ofstream prints doubles by default (%g, 6 significant digits)."""
    t_beg = traj.t0_ns * 1e-9
    dt = traj.dt_ns * 1e-9
    with open(path, "w") as f:
        for i, q in enumerate(traj.knots_xyzw):
            f.write("%g 0 0 0 %g %g %g %g\n" % (t_beg + i * dt - time_offset, q[0], q[1], q[2], q[3]))


# ---- control poses --------------------------------------------------------------------------------------------------------
def fit_ctrl_poses(t, qs, t_beg, dt_knots, num_cps):
    """LinearTrajectory::fitCtrlPoses: lift to the tangent space at the first pose, solve N P = D for the control points of the
    uniform linear spline (basis [1-u, u]), retract."""
    if len(t) < num_cps:
        raise ValueError("fewer poses than control poses")                     # CHECK_GE
    offset = qs[0]
    off_inv = so3.inverse(offset)
    N = np.zeros((len(t), num_cps))
    D = np.zeros((len(t), 3))
    for k, (tk, qk) in enumerate(zip(t, qs)):
        ti = int(np.floor((tk - t_beg) / dt_knots))
        u = (tk - (ti * dt_knots + t_beg)) / dt_knots
        N[k, ti] = 1.0 - u                                                     # U * M2 with M2 = [[1,0],[-1,1]]
        if ti + 1 < num_cps:
            N[k, ti + 1] = u
        D[k] = so3.log(so3.mul(off_inv, qk))
    P = np.linalg.lstsq(N, D, rcond=None)[0]                                   # fullPivHouseholderQr().solve
    return np.array([so3.mul(offset, so3.exp(P[i])) for i in range(num_cps)])


def generate_ctrl_poses_long(t, qs, t_beg, t_end, dt_knots, sub_interval_length):
    n_sub = int(np.floor((t_end - t_beg) / sub_interval_length + 1e-6))
    out = []
    for i in range(n_sub):
        a = t_beg + sub_interval_length * i
        b = a + sub_interval_length
        sel = (t > a) & (t < b)                                                # upper_bound(a) .. lower_bound(b)
        num_cps = int(round((b - a) / dt_knots)) + 1
        cps = fit_ctrl_poses(t[sel], qs[sel], a, dt_knots, num_cps)
        out.extend(cps[1:] if i else cps)
    return np.array(out)


def incremental_update(traj, x1, fix_first_pose):
    """Model::updateTraj + LinearTrajectory::incrementalUpdate (model.cpp:22-53, trajectory.cpp:296-304): knot_i <- exp(x1_i) * knot_i.
    x1 has 3K entries (zeros for a fixed first pose, as emba_solve_normal_eq returns it).  All control poses at once (numpy; the same
    Sophus formulas as so3.exp / so3.mul: so3.hpp:583-619, 324-339) — the per-pose Python loop was 1.1 ms of a 8.4-ms LM iteration at K = 201."""
    knots = traj.knots_xyzw.copy()
    s = 1 if fix_first_pose else 0
    w = np.asarray(x1, dtype=np.float64).reshape(-1, 3)[s:len(knots)]
    th2 = (w * w).sum(axis=1)
    small = th2 < so3.EPS * so3.EPS
    th = np.sqrt(np.where(small, 1.0, th2))
    imag = np.where(small, 0.5 - th2 / 48.0 + th2 * th2 / 3840.0, np.sin(0.5 * th) / th)
    real = np.where(small, 1.0 - th2 / 8.0 + th2 * th2 / 384.0, np.cos(0.5 * th))
    ax, ay, az, aw = imag * w[:, 0], imag * w[:, 1], imag * w[:, 2], real
    bx, by, bz, bw = knots[s:, 0], knots[s:, 1], knots[s:, 2], knots[s:, 3]
    q = np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                  aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], axis=1)
    knots[s:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return LinearTrajectory(knots, traj.t0_ns, traj.dt_ns)


# ---- camera ---------------------------------------------------------------------------------------------------------------
def bearing_lut_from_calibration(K, D, width, height, iters=5):
    """Bearing vector (x', y', 1) of every sensor pixel, row-major [height*width, 3], for a monocular plumb_bob camera (R = I,
    P = [K | 0]): rectifyPoint undistorts the pixel (cv::undistortPoints: fixed-point iteration on the radial-tangential model,
    5 iterations) and re-projects with K; projectPixelTo3dRay maps that back through K, so the ray is the undistorted normalised
    point.  image_geometry / OpenCV are not part of the reference tree: published algorithm, parity unpinned."""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    D = np.zeros(5) if D is None else np.concatenate([np.asarray(D, dtype=np.float64).ravel(), np.zeros(5)])[:5]
    k1, k2, p1, p2, k3 = D
    v, u = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    x0 = (u - K[0, 2]) / K[0, 0]
    y0 = (v - K[1, 2]) / K[1, 1]
    x, y = x0.copy(), y0.copy()
    for _ in range(iters):
        r2 = x * x + y * y
        icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = (x0 - dx) * icdist
        y = (y0 - dy) * icdist
    return np.ascontiguousarray(np.stack([x, y, np.ones_like(x)], axis=-1).reshape(-1, 3))


# ---- display images ---------------------------------------------------------------------------------------------------------
def normalize_robust(img, percentage_pixels_to_discard=0.1):
    """image_util::normalizeRobust: scale [robust min, robust max] (order statistics after discarding the given percentage of
    pixels, float32 index arithmetic like the reference) to [0, 255]; cv::Mat::convertTo(CV_8UC1) = round half to even, saturate."""
    a = np.asarray(img, dtype=np.float64)
    rmin, rmax = robust_range(a, percentage_pixels_to_discard)
    scale = 255.0 / (rmax - rmin) if rmax != rmin else 1.0
    return np.clip(np.rint(scale * (a - rmin)), 0, 255).astype(np.uint8)


def robust_range(img, percentage_pixels_to_discard=0.1):
    """image_util::minMaxLocRobust (image_utils.cpp:22-23): the order statistics normalize_robust scales between, (rmin, rmax) — what
    LEGM.normalizeRobust(with_range=True) returns beside the image."""
    a = np.asarray(img, dtype=np.float64)
    srt = np.sort(a, axis=None)
    n = a.size
    i_min = int(np.float32(np.float32(0.5) * np.float32(percentage_pixels_to_discard) / np.float32(100.0)) * np.float32(n))
    i_max = int(np.float32(np.float32(1.0) - np.float32(0.5) * np.float32(percentage_pixels_to_discard) / np.float32(100.0)) * np.float32(n))
    return float(srt[i_min]), float(srt[min(i_max, n - 1)])


def save_pgm(path, img_u8):
    img_u8 = np.ascontiguousarray(img_u8, dtype=np.uint8)
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img_u8.shape[1], img_u8.shape[0]))
        f.write(img_u8.tobytes())


def load_pgm(path):
    """A binary PGM (P5) as an array [h, w]: uint8 where maxval < 256, else big-endian uint16.  The header is magic, width, height, maxval, separated by
    whitespace, with '#' comments; one whitespace byte in front of the raster.  What save_pgm writes, read back."""
    with open(path, "rb") as f:
        raw = f.read()
    tok, pos = [], 0
    while len(tok) < 4:
        while raw[pos:pos + 1].isspace():
            pos += 1
        if raw[pos:pos + 1] == b"#":
            pos = raw.index(b"\n", pos) + 1
            continue
        end = pos
        while end < len(raw) and not raw[end:end + 1].isspace():
            end += 1
        if end == pos:
            raise ValueError(f"{path}: the PGM header ends early")
        tok.append(raw[pos:end]); pos = end
    if tok[0] != b"P5":
        raise ValueError(f"{path}: not a binary PGM")
    w, h, maxval = int(tok[1]), int(tok[2]), int(tok[3])
    return np.frombuffer(raw, dtype=np.uint8 if maxval < 256 else ">u2", count=w * h, offset=pos + 1).reshape(h, w)


def save_png(path, img_u8, level=1):
    """8-bit greyscale (H x W) or RGB (H x W x 3) PNG: filter type 0 on every row, deflated with the standard library's zlib at `level`."""
    import struct
    import zlib
    a = np.ascontiguousarray(img_u8, dtype=np.uint8)
    if a.ndim == 2:
        color, ch = 0, 1
    elif a.ndim == 3 and a.shape[2] == 3:
        color, ch = 2, 3
    else:
        raise ValueError(f"save_png takes H x W or H x W x 3 uint8, not {a.shape}")
    h, w = a.shape[:2]
    raw = np.empty((h, 1 + w * ch), np.uint8)
    raw[:, 0] = 0
    raw[:, 1:] = a.reshape(h, w * ch)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, color, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(raw.tobytes(), level)))
        f.write(chunk(b"IEND", b""))


# ---- events ---------------------------------------------------------------------------------------------------------------
def save_events(path, events):
    np.savez_compressed(path, x=np.asarray(events.x, np.uint16), y=np.asarray(events.y, np.uint16),
                        polarity=np.asarray(events.polarity, np.uint8), t_ns=np.asarray(events.t_ns, np.int64))


def load_events(path, t_min_ns=None, t_max_ns=None):
    """Events in [t_min, t_max], sorted by timestamp (stable) like parse_rosbag's std::sort (rosbag_loading.cpp:61-65)."""
    d = np.load(path)
    x, y, p, t = d["x"], d["y"], d["polarity"], d["t_ns"]
    order = np.argsort(t, kind="stable")
    x, y, p, t = x[order], y[order], p[order], t[order]
    sel = np.ones(t.size, bool)
    if t_min_ns is not None:
        sel &= t >= t_min_ns
    if t_max_ns is not None:
        sel &= t <= t_max_ns
    return EventPacket(x[sel], y[sel], p[sel], t[sel])


# ---- the sequence-level steps of EMBA::EMBA / EMBA::Run (numpy forms; the device forms are LEGM.set_sequence / sequence_window / median_blur_map) ------
def ros_time_ns(t_sec):
    """ros::Time(double) / ros::Duration(double) as integer nanoseconds (fromSec: sec = floor(t), nsec = round((t - sec) * 1e9), carried)."""
    sec = int(np.floor(t_sec))
    return sec * 1_000_000_000 + int(np.round((t_sec - sec) * 1e9))


def downsample_events(events, rate):
    """emba.cpp:281-304: with rate >= 2 exactly the events with index rate-1, 2 rate-1, ... survive (n // rate of them); otherwise all."""
    rate = int(rate)
    if rate < 2:
        return events
    sl = slice(rate - 1, None, rate)
    return EventPacket(events.x[sl], events.y[sl], events.polarity[sl], events.t_ns[sl])


def event_window(t_ns, t_beg_ns, t_end_ns):
    """EMBA::getEventSubset (emba.cpp:473-510) on sorted timestamps: (beg, end) of the subset, both cursors moving 100 events at a time behind the
    1-ms margins.  Raises ValueError where the reference's tail search stops at its first probe (its `-= 100` underflows size_t) or the subset would be a
    reversed range — "window holds no events", as emba_seq_window reports it."""
    t = np.asarray(t_ns, dtype=np.int64)
    n = t.size
    a, b = int(t_beg_ns) + 1_000_000, int(t_end_ns) - 1_000_000              # :476-478
    probes = t[::100]
    m = probes.size
    jb = int(np.searchsorted(probes, a, side="right"))                       # :483-491: the first probe later than a
    beg, end = 100 * jb, n
    if jb < m:
        je = max(int(np.searchsorted(probes, b, side="right")), jb)          # :494-503, starting from the head
        if je < m:
            if je == jb:
                raise ValueError(f"window holds no events (the tail search stops at its first probe, event {beg})")
            end = 100 * je - 100
    if beg > end:
        raise ValueError("window holds no events (it begins behind the last event)")
    return beg, end


def slice_events(events, beg, end):
    return EventPacket(events.x[beg:end], events.y[beg:end], events.polarity[beg:end], events.t_ns[beg:end])


def median_blur3(plane):
    """emba.cpp:357-364 for one plane: float32 copy (round to nearest even), 3x3 median with replicated borders (cv::BORDER_REPLICATE),
    back to float64.  The median is one of the nine values, so the device form (emba_median_blur3) gives the same numbers."""
    a = np.asarray(plane, dtype=np.float64).astype(np.float32)
    h, w = a.shape
    p = np.pad(a, 1, mode="edge")
    nine = np.stack([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)])
    return np.sort(nine, axis=0)[4].astype(np.float64)


# ---- sensor noise (numpy form of emba_seq_filter, include/emba_hip.h; the device form is LEGM.filter_sequence) --------------------------------------
def hot_pixel_threshold(counts, hot_sigma):
    """mean + hot_sigma * sqrt(var) of the event counts of the pixels that have events, from exact integer sums; python floats: every operation is
    rounded on its own, as the rule demands."""
    c = np.asarray(counts)
    c = c[c > 0].astype(np.uint64)
    m, s1, s2 = int(c.size), int(c.sum(dtype=np.uint64)), int((c * c).sum(dtype=np.uint64))
    mean = float(s1) / float(m)
    var = float(s2) / float(m) - mean * mean
    if var < 0.0:
        var = 0.0
    return mean + float(hot_sigma) * float(np.sqrt(var))


def filter_events(events, sensor_w, sensor_h, hot_sigma=0.0, refractory_ns=0, support_ns=0):
    """Hot-pixel, refractory and neighbour-support filters on a whole recording (sorted by time), each event judged from the RAW sequence: the rule of
    emba_seq_filter, vectorised — one stable sort by sensor pixel, then one searchsorted per neighbouring pixel.  Returns (events, stats, hot_mask):
    the survivors in their order (the SAME packet when every filter is off), stats = uint64[6] (events in, hot pixels, events failing hot, failing
    refractory, failing support, survivors) and hot_mask = uint8[sensor_w * sensor_h].  No down-sampling here: downsample_events of the result."""
    sw, sh = int(sensor_w), int(sensor_h)
    S = sw * sh
    hot_sigma, refractory_ns, support_ns = float(hot_sigma), int(refractory_ns), int(support_ns)
    if np.isnan(hot_sigma):
        raise ValueError("hot_sigma is NaN")
    x, y = np.asarray(events.x, dtype=np.int64), np.asarray(events.y, dtype=np.int64)
    t = np.asarray(events.t_ns, dtype=np.int64)
    n = t.size
    stats = np.zeros(6, dtype=np.uint64)
    stats[0] = stats[5] = n
    hot = np.zeros(S, dtype=bool)
    if n == 0 or not (hot_sigma > 0 or refractory_ns > 0 or support_ns > 0):
        return events, stats, hot.astype(np.uint8)
    if (x >= sw).any() or (y >= sh).any():
        raise ValueError(f"an event lies outside the {sw}x{sh} sensor")
    pix = y * sw + x
    order = np.argsort(pix, kind="stable")                     # (pixel, index): every pixel's events in index order, end to end
    sp = pix[order]
    counts = np.bincount(pix, minlength=S)
    start = np.concatenate([[0], np.cumsum(counts)])
    if hot_sigma > 0:
        hot = counts.astype(np.float64) > hot_pixel_threshold(counts, hot_sigma)
    fail_hot = hot[pix]
    fail_ref = np.zeros(n, dtype=bool)
    if refractory_ns > 0:
        f = (sp[1:] == sp[:-1]) & (t[order[1:]] - t[order[:-1]] < refractory_ns)
        fail_ref[order[1:][f]] = True
    fail_sup = np.zeros(n, dtype=bool)
    if support_ns > 0:
        comp = sp * n + order                                  # ascending: (pixel, index) as one integer
        k = np.arange(n, dtype=np.int64)
        ok = np.zeros(n, dtype=bool)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == 0 and dy == 0:
                    continue
                qx, qy = x + dx, y + dy
                valid = (qx >= 0) & (qx < sw) & (qy >= 0) & (qy < sh)
                q = np.where(valid, qy * sw + qx, 0)
                valid &= ~hot[q]
                j = np.searchsorted(comp, q * n + k) - 1      # the last entry of (pixel q, index < k), if it lies in q's chain
                valid &= j >= start[q]
                ok |= valid & (t - t[order[np.maximum(j, 0)]] <= support_ns)
        fail_sup = ~ok
    keep = ~(fail_hot | fail_ref | fail_sup)
    stats[1], stats[2], stats[3], stats[4], stats[5] = int(hot.sum()), int(fail_hot.sum()), int(fail_ref.sum()), int(fail_sup.sum()), int(keep.sum())
    out = EventPacket(np.asarray(events.x)[keep], np.asarray(events.y)[keep], np.asarray(events.polarity)[keep], np.asarray(events.t_ns)[keep])
    return out, stats, hot.astype(np.uint8)


# ---- angular velocity from the events alone: contrast maximisation (numpy form of emba_seq_cmax / emba_seq_cmax_objective, include/emba_hip.h; the
# device forms are LEGM.estimate_angular_velocity / LEGM.cmax_objective).  The rule — grid, pinhole, warp, votes, search — is emba_amd/csrc/cmax_rule.h's
# and cmax_kernels.h's, operation for operation: J and the image are integers, so both forms give the same bits.
CMAX_GRID_CELLS = (64 << 10) // 4        # kCmaxMaxCells: the uint32 cells that fit 64 KiB
CMAX_MAX_RANGE = (1 << 24) - 1           # kCmaxMaxRange: events a 32-bit cell counts exactly
CMAX_MAX_ITER = 64                       # kCmaxMaxIter


def cmax_grid(sensor_w, sensor_h):
    """(shift, grid_w, grid_h): cells of 2^shift sensor pixels, shift the smallest for which the grid of uint32 cells fits 64 KiB (cmax_rule.h: cmax_grid)."""
    s = 0
    while True:
        gw, gh = (int(sensor_w) + (1 << s) - 1) >> s, (int(sensor_h) + (1 << s) - 1) >> s
        if gw * gh <= CMAX_GRID_CELLS:
            return s, gw, gh
        s += 1


def _cmax_fit_line(lut, first, stride, count, comp):
    """cmax_rule.h: cmax_fit_line — python floats, every operation rounded on its own, the sums in index order."""
    pts = []
    for i in range(count):
        b = lut[first + i * stride]
        if not float(b[2]) > 0.0:
            continue
        pts.append((float(i), float(b[comp]) / float(b[2])))
    if not pts:
        return 0.0, 0.0, 0.0, False
    sp = sr = 0.0
    for p, r in pts:
        sp = sp + p
        sr = sr + r
    m_pos, m_ratio = sp / float(len(pts)), sr / float(len(pts))
    spr = srr = 0.0
    for p, r in pts:
        dp, dr = p - m_pos, r - m_ratio
        spr = spr + dp * dr
        srr = srr + dr * dr
    if len(pts) < 2 or not srr > 0.0:
        return m_pos, m_ratio, 0.0, False
    slope = spr / srr
    return m_pos, m_ratio, slope, bool(np.isfinite(slope) and slope > 0.0)


def cmax_pinhole_fit(lut, sensor_w, sensor_h):
    """(f, cu, cv) of the ideal pinhole u = f b'x / b'z + cu, v = f b'y / b'z + cv behind the image of warped events: least squares of x over b.x / b.z
    along the LUT's centre row and of y over b.y / b.z along its centre column (cmax_rule.h: cmax_pinhole_fit, the same operations in the same order).
    Raises ValueError where neither line has a positive slope."""
    sw, sh = int(sensor_w), int(sensor_h)
    lut = np.asarray(lut, dtype=np.float64).reshape(sw * sh, 3)
    rp, rr, rs, rok = _cmax_fit_line(lut, (sh // 2) * sw, 1, sw, 0)
    cp, cr, cs, cok = _cmax_fit_line(lut, sw // 2, sw, sh, 1)
    if not rok and not cok:
        raise ValueError("the bearing LUT has no pinhole fit")
    f = (rs + cs) * 0.5 if (rok and cok) else (rs if rok else cs)
    cu, cv = rp - f * rr, cp - f * cr
    if not (np.isfinite(f) and np.isfinite(cu) and np.isfinite(cv)):
        raise ValueError("the bearing LUT has no pinhole fit")
    return f, cu, cv


def cmax_objective(events, lut, sensor_w, sensor_h, omega, beg=0, end=None, want_iwe=True, pinhole=None):
    """J(w) = sum of I^2 over the image of warped events of events[beg:end], t_ref = t[beg], for every candidate of omega [M, 3]: (J uint64 [M],
    iwe uint32 [M, grid_h, grid_w] or None).  The rule of emba_seq_cmax_objective (include/emba_hip.h), vectorised over the events."""
    sw, sh = int(sensor_w), int(sensor_h)
    shift, gw, gh = cmax_grid(sw, sh)
    f, cu, cv = pinhole if pinhole is not None else cmax_pinhole_fit(lut, sw, sh)
    lut = np.asarray(lut, dtype=np.float64).reshape(sw * sh, 3)
    omega = np.asarray(omega, dtype=np.float64).reshape(-1, 3)
    if not np.isfinite(omega).all():
        raise ValueError("omega is not finite")
    n = int(np.asarray(events.t_ns).size)
    end = n if end is None else int(end)
    beg = int(beg)
    if not 0 <= beg <= end <= n:
        raise ValueError(f"[{beg}, {end}) is not a range of the sequence of {n} events")
    if end - beg > CMAX_MAX_RANGE:
        raise ValueError(f"[{beg}, {end}): the 32-bit cells of the image count at most {CMAX_MAX_RANGE} events exactly")
    M, cells = omega.shape[0], gw * gh
    J = np.zeros(M, dtype=np.uint64)
    iwe = np.zeros((M, gh, gw), dtype=np.uint32) if want_iwe else None
    if beg == end:
        return J, iwe
    t = np.asarray(events.t_ns, dtype=np.int64)[beg:end]
    p = np.asarray(events.y, dtype=np.int64)[beg:end] * sw + np.asarray(events.x, dtype=np.int64)[beg:end]
    b0, b1, b2 = lut[p, 0], lut[p, 1], lut[p, 2]
    hdt = ((t - t[0]).astype(np.float64) * 1e-9) * 0.5
    inv = 1.0 / float(1 << shift)
    for j in range(M):
        a0, a1, a2 = omega[j, 0] * hdt, omega[j, 1] * hdt, omega[j, 2] * hdt
        aa = (a0 * a0 + a1 * a1) + a2 * a2
        c0, c1, c2 = a1 * b2 - a2 * b1, a2 * b0 - a0 * b2, a0 * b1 - a1 * b0
        d0, d1, d2 = a1 * c2 - a2 * c1, a2 * c0 - a0 * c2, a0 * c1 - a1 * c0
        s = 1.0 + aa
        r0, r1, r2 = s * b0 + 2.0 * (c0 + d0), s * b1 + 2.0 * (c1 + d1), s * b2 + 2.0 * (c2 + d2)
        with np.errstate(all="ignore"):
            front = r2 > 0.0
            r2s = np.where(front, r2, 1.0)
            gx, gy = (f * (r0 / r2s) + cu) * inv, (f * (r1 / r2s) + cv) * inv
            ok = front & (gx >= -1.0) & (gx < float(gw)) & (gy >= -1.0) & (gy < float(gh))
        gx, gy = gx[ok], gy[ok]
        fx, fy = np.floor(gx), np.floor(gy)
        ix, iy = fx.astype(np.int64), fy.astype(np.int64)
        wx, wy = ((gx - fx) * 16.0).astype(np.int64), ((gy - fy) * 16.0).astype(np.int64)
        acc = np.zeros(cells, dtype=np.float64)         # (sums of integers below 2^32: exact in a double)
        for dx, dy, v in ((0, 0, (16 - wx) * (16 - wy)), (1, 0, wx * (16 - wy)), (0, 1, (16 - wx) * wy), (1, 1, wx * wy)):
            cx, cy = ix + dx, iy + dy
            ins = (cx >= 0) & (cx < gw) & (cy >= 0) & (cy < gh)
            acc += np.bincount((cy * gw + cx)[ins], weights=v[ins].astype(np.float64), minlength=cells)
        I = acc.astype(np.uint64)
        J[j] = (I * I).sum(dtype=np.uint64)
        if want_iwe:
            iwe[j] = I.astype(np.uint32).reshape(gh, gw)
    return J, iwe


def cmax_search(J_of, omega_max):
    """The compass search of one slice (cmax_rule.h: CmaxSearch) over J_of(omega [6, 3]) -> six integers: (omega [3], J0, J, evaluations); J_of is first
    asked for omega = 0 alone.  same_instant slices are the caller's."""
    w = [0.0, 0.0, 0.0]
    J0 = J = int(J_of(np.zeros((1, 3)))[0])
    step, min_step, it, evals = omega_max * 0.5, omega_max * (1.0 / 4096.0), 0, 1
    while it < CMAX_MAX_ITER and not step < min_step:
        cand = np.array([w] * 6)
        for c in range(6):
            cand[c, c >> 1] = w[c >> 1] + (-1.0 if c & 1 else 1.0) * step
        Jc = [int(v) for v in J_of(cand)]
        evals += 6
        best = max(range(6), key=lambda c: (Jc[c], -c))      # ties: the earlier candidate
        if Jc[best] > J:
            w, J = [float(v) for v in cand[best]], Jc[best]
        else:
            step = step * 0.5
        it += 1
    return w, J0, J, evals


def estimate_angular_velocity(events, lut, sensor_w, sensor_h, slice_events, omega_max):
    """The angular velocity of every slice of slice_events events by contrast maximisation: the rule of emba_seq_cmax (include/emba_hip.h) in numpy, for
    models without a resident sequence and for the tests.  Returns a dict: omega float64 [n_slices, 3] (rad/s, body frame), t_ref_ns int64 [n_slices + 1]
    (every slice's first timestamp, then the last estimated event's; empty where n_slices = 0), J0, J uint64 [n_slices], evals int32 [n_slices]."""
    m, omega_max = int(slice_events), float(omega_max)
    if m < 1:
        raise ValueError(f"slice_events = {m}: a slice has at least one event")
    if not (np.isfinite(omega_max) and omega_max > 0.0):
        raise ValueError("omega_max must be finite and positive")
    if m > CMAX_MAX_RANGE:
        raise ValueError(f"slice_events = {m}: the 32-bit cells of the image count at most {CMAX_MAX_RANGE} events exactly")
    t = np.asarray(events.t_ns, dtype=np.int64)
    ns = t.size // m
    out = dict(omega=np.zeros((ns, 3)), t_ref_ns=np.zeros(ns + 1 if ns else 0, np.int64), J0=np.zeros(ns, np.uint64), J=np.zeros(ns, np.uint64),
               evals=np.zeros(ns, np.int32))
    if not ns:
        return out
    pin = cmax_pinhole_fit(lut, sensor_w, sensor_h)
    out["t_ref_ns"][:ns], out["t_ref_ns"][ns] = t[0:ns * m:m], t[ns * m - 1]
    for s in range(ns):
        beg, end = s * m, (s + 1) * m
        J_of = lambda w: cmax_objective(events, lut, sensor_w, sensor_h, w, beg, end, want_iwe=False, pinhole=pin)[0]
        if t[end - 1] == t[beg]:
            w, J0, evals = [0.0, 0.0, 0.0], int(J_of(np.zeros((1, 3)))[0]), 1
            J = J0
        else:
            w, J0, J, evals = cmax_search(J_of, omega_max)
        out["omega"][s], out["J0"][s], out["J"][s], out["evals"][s] = w, J0, J, evals
    return out


def integrate_angular_velocity(omega, t_ref_ns, t_query_ns=None):
    """The rotation that per-slice angular velocities describe: q_0 = identity, q_{s+1} = q_s * exp(omega_s (t_ref(s+1) - t_ref(s))) (so3.exp; body frame,
    the convention of warpEventToMap's R * bearing), t_ref_ns [n_slices + 1] as estimate_angular_velocity returns it — the last interval ends at the last
    estimated event and uses the last omega.  Returns (pose_t [n_slices + 1] seconds, pose_q [n_slices + 1, 4] xyzw): what load_poses returns, what
    generate_ctrl_poses_long consumes.  With t_query_ns: (t seconds, q) at those times instead, slice s = the last one beginning at or before t (the first /
    last slice's velocity outside the estimated span)."""
    omega = np.asarray(omega, dtype=np.float64).reshape(-1, 3)
    t_ref = np.asarray(t_ref_ns, dtype=np.int64)
    ns = omega.shape[0]
    if ns == 0:
        raise ValueError("no slice was estimated")
    if t_ref.size != ns + 1:
        raise ValueError(f"{ns} slices need {ns + 1} reference times, not {t_ref.size}")
    q = np.zeros((ns + 1, 4))
    q[0] = (0.0, 0.0, 0.0, 1.0)
    for s in range(ns):
        q[s + 1] = so3.mul(q[s], so3.exp(omega[s] * (float(t_ref[s + 1] - t_ref[s]) * 1e-9)))
    if t_query_ns is None:
        return t_ref * 1e-9, q
    tq = np.asarray(t_query_ns, dtype=np.int64)
    sl = np.clip(np.searchsorted(t_ref[:ns], tq, side="right") - 1, 0, ns - 1)
    return tq * 1e-9, np.array([so3.mul(q[s], so3.exp(omega[s] * (float(tk - t_ref[s]) * 1e-9))) for s, tk in zip(sl, tq)]).reshape(-1, 4)


# ---- the panorama of warped events along a trajectory and its contrast (numpy form of emba_seq_event_panorama, include/emba_hip.h; the device form is
# LEGM.event_panorama).  The votes are emba_amd/csrc/panorama_rule.h's pano_vote, operation for operation: given the same pm both forms give the same integers.
PANO_BATCH = 100                         # kPanoBatch: events per pose (model.cpp:100-119)
PANO_MAX_EVENTS = 1 << 23                # kPanoMaxEvents: a range of this many used events or more is refused


def pano_votes(pm, pano_w, pano_h):
    """pano_vote (panorama_rule.h) of every row of pm [n, 2]: (cell int64 [n, 4], weight int64 [n, 4]) for the cells (ix, iy), (ix + 1, iy), (ix, iy + 1),
    (ix + 1, iy + 1) — cell = row * pano_w + column with the column wrapped modulo pano_w, -1 where the row lies outside [0, pano_h); a pm that is not
    finite (or |pm| >= 2^31) has every cell -1 and every weight 0."""
    W, H = int(pano_w), int(pano_h)
    pm = np.asarray(pm, dtype=np.float64).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(pm[:, 0]) < 2147483648.0) & (np.abs(pm[:, 1]) < 2147483648.0)
    x, y = np.where(ok, pm[:, 0], 0.0), np.where(ok, pm[:, 1], 0.0)
    fx, fy = np.floor(x), np.floor(y)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    wx, wy = ((x - fx) * 16.0).astype(np.int64), ((y - fy) * 16.0).astype(np.int64)
    c0 = ix % W
    c1 = np.where(c0 + 1 == W, 0, c0 + 1)
    r0, r1 = (iy >= 0) & (iy < H) & ok, (iy + 1 >= 0) & (iy + 1 < H) & ok
    cell = np.stack([np.where(r0, iy * W + c0, -1), np.where(r0, iy * W + c1, -1), np.where(r1, (iy + 1) * W + c0, -1), np.where(r1, (iy + 1) * W + c1, -1)], axis=1)
    w = np.stack([(16 - wx) * (16 - wy), wx * (16 - wy), (16 - wx) * wy, wx * wy], axis=1) * ok[:, None]
    return cell, w


def event_panorama_pm(events, lut, sensor_w, sensor_h, pano_w, pano_h, traj, beg=0, end=None):
    """pm [nn, 2] of the used events of events[beg:end] (whole batches of 100) along traj: batch b of the range takes the spline pose at its midpoint
    (sharded.batch_mid_ns of its first and last timestamp, model.cpp:116-119; so3.spline_evaluate), pm = project(R * bearing) with the equirectangular
    projection of synth.project_equirect.  numpy's sin / atan2 / asin are not the device's: close to emba_seq_event_panorama's pm_out, not bit-equal.
    Raises ValueError where a midpoint lies outside the knots."""
    from . import synth
    from .sharded import batch_mid_ns
    sw = int(sensor_w)
    lut = np.asarray(lut, dtype=np.float64).reshape(sw * int(sensor_h), 3)
    t = np.asarray(events.t_ns, dtype=np.int64)
    end = t.size if end is None else int(end)
    beg = int(beg)
    if not 0 <= beg <= end <= t.size:
        raise ValueError(f"[{beg}, {end}) is not a range of the sequence of {t.size} events")
    nb = (end - beg) // PANO_BATCH
    nn = nb * PANO_BATCH
    p = np.asarray(events.y, dtype=np.int64)[beg:beg + nn] * sw + np.asarray(events.x, dtype=np.int64)[beg:beg + nn]
    pm = np.zeros((nn, 2))
    for b in range(nb):
        k0 = beg + PANO_BATCH * b
        q = so3.spline_evaluate(traj.knots_xyzw, traj.t0_ns, traj.dt_ns, batch_mid_ns(t[k0], t[k0 + PANO_BATCH - 1]))
        rb = lut[p[PANO_BATCH * b:PANO_BATCH * (b + 1)]] @ synth._quat_to_R(q).T
        pm[PANO_BATCH * b:PANO_BATCH * (b + 1), 0], pm[PANO_BATCH * b:PANO_BATCH * (b + 1), 1] = synth.project_equirect(int(pano_w), int(pano_h), rb)
    return pm


def event_panorama(events, lut, sensor_w, sensor_h, pano_w, pano_h, traj, beg=0, end=None, signed=False, pm=None):
    """The panorama of warped events of events[beg:end] along the linear SO(3) spline traj, and its contrast: the rule of emba_seq_event_panorama
    (include/emba_hip.h) in numpy.  Returns a dict: image int64 [pano_h, pano_w], J = sum I^2, sum = sum I, nonzero = cells != 0, dropped = votes (non-zero
    weights) whose row lies outside the panorama — python ints — and pm float64 [nn, 2], nn = ((end - beg) // 100) * 100.
    Given pm [nn, 2] (the device's pm_out, an oracle's) the integer rule is applied to it exactly: the same image, bit for bit, as the device makes of the
    same pm.  Without pm it is computed here (event_panorama_pm): numpy's sin / atan2 / asin differ from the device's in the last bits, so that image is
    close to the device's but not bit-equal (DESIGN.md §12 has the measured distance).  traj may be None where pm is given."""
    W, H = int(pano_w), int(pano_h)
    n = int(np.asarray(events.t_ns).size)
    end = n if end is None else int(end)
    beg = int(beg)
    if not 0 <= beg <= end <= n:
        raise ValueError(f"[{beg}, {end}) is not a range of the sequence of {n} events")
    nn = ((end - beg) // PANO_BATCH) * PANO_BATCH
    if nn >= PANO_MAX_EVENTS:
        raise ValueError(f"[{beg}, {end}): the 32-bit cells of the image count fewer than {PANO_MAX_EVENTS} events exactly")
    if pm is None:
        if traj is None or traj.size() < 2 or int(traj.dt_ns) <= 0:
            raise ValueError("event_panorama needs a trajectory of at least two control poses with a positive knot spacing, or pm")
        pm = event_panorama_pm(events, lut, sensor_w, sensor_h, W, H, traj, beg, end)
    pm = np.asarray(pm, dtype=np.float64).reshape(-1, 2)
    if pm.shape[0] != nn:
        raise ValueError(f"pm has {pm.shape[0]} rows, the range uses {nn} events")
    cell, w = pano_votes(pm, W, H)
    if signed:
        w = np.where((np.asarray(events.polarity)[beg:beg + nn] == 0)[:, None], -w, w)
    inside = cell >= 0
    acc = np.bincount(cell[inside], weights=w[inside].astype(np.float64), minlength=W * H)      # (sums of integers below 2^31: exact in a double)
    image = acc.astype(np.int64).reshape(H, W)
    return dict(pano_contrast(image), image=image, dropped=int(np.count_nonzero(~inside & (w != 0))), pm=pm)


def pano_contrast(image):
    """J = sum I^2, sum = sum I, nonzero = cells != 0 of an image of warped events, as python ints.  With sum |I| < 2^31 (one call's image) every sum is
    exact in int64; the sum of several calls' images may exceed that, and its squares are then added as python ints."""
    image = np.asarray(image, dtype=np.int64)
    nz = image[image != 0]
    J = int((nz * nz).sum()) if int(np.abs(nz).sum()) < (1 << 31) else sum(int(v) * int(v) for v in nz.tolist())
    return dict(J=J, sum=int(image.sum()), nonzero=int(nz.size))


# ---- the smooth contrast of that panorama and its gradient with respect to the control poses (numpy form of emba_seq_contrast_gradient, include/emba_hip.h,
# given pm, D and cp; the device form is LEGM.contrast_gradient).  The votes are emba_amd/csrc/contrast_rule.h's contrast_vote, operation for operation.
def contrast_votes(pm, pano_w, pano_h):
    """contrast_vote (contrast_rule.h) of every row of pm [n, 2]: (cell int64 [n, 4], w, dwx, dwy float64 [n, 4]) for the cells (ix, iy), (ix + 1, iy),
    (ix, iy + 1), (ix + 1, iy + 1) — the bilinear weights (1 - ax)(1 - ay), ax (1 - ay), (1 - ax) ay, ax ay and their derivatives in pm_x and pm_y; cell =
    row * pano_w + column with the column wrapped modulo pano_w, -1 where the row lies outside [0, pano_h); a pm that is not finite (or |pm| >= 2^31) has
    every cell -1 and every weight and derivative 0."""
    W, H = int(pano_w), int(pano_h)
    pm = np.asarray(pm, dtype=np.float64).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(pm[:, 0]) < 2147483648.0) & (np.abs(pm[:, 1]) < 2147483648.0)
    x, y = np.where(ok, pm[:, 0], 0.0), np.where(ok, pm[:, 1], 0.0)
    fx, fy = np.floor(x), np.floor(y)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    ax, ay = x - fx, y - fy
    bx, by = 1.0 - ax, 1.0 - ay
    c0 = ix % W
    c1 = np.where(c0 + 1 == W, 0, c0 + 1)
    r0, r1 = (iy >= 0) & (iy < H) & ok, (iy + 1 >= 0) & (iy + 1 < H) & ok
    cell = np.stack([np.where(r0, iy * W + c0, -1), np.where(r0, iy * W + c1, -1), np.where(r1, (iy + 1) * W + c0, -1), np.where(r1, (iy + 1) * W + c1, -1)], axis=1)
    m = ok[:, None]
    w = np.stack([bx * by, ax * by, bx * ay, ax * ay], axis=1) * m
    dwx = np.stack([-by, by, -ay, ay], axis=1) * m
    dwy = np.stack([-bx, -ax, bx, ax], axis=1) * m
    return cell, w, dwx, dwy


def contrast_gradient(pm, D, cp, pol, K, pano_w, pano_h, signed=False, prior=None):
    """The smooth contrast of the panorama of warped events and its gradient, given what the warp produced: pm [n, 2], D [n, 2, 6] (dpm_ddrot_cp, J23
    [I - J1 | J1]), cp [n] (the control pose the event's spline segment begins at) and pol [n] (None: every event votes positive).  Returns a dict: image
    float64 [pano_h, pano_w], J = sum I^2, grad float64 [3 K] with respect to the increments of incremental_update (ge = 2 s gp^T D per event, gp = sum over
    the kept cells of I(c) (dwx, dwy); ge[0:3] to control pose cp, ge[3:6] to cp + 1; a component that is not finite, or an event whose cp lies outside
    [0, K - 2], adds nothing), dropped = votes (non-zero weights) whose row lies outside the panorama.  D and cp may be None: grad is then None.
    prior: None, or an array [pano_h, pano_w] the image starts from instead of zeros — what earlier events voted, times its weight (the caller passes
    lambda P: the numpy form of emba_seq_contrast_gradient_prior); J and the gradient are then those of that image."""
    W, H, K = int(pano_w), int(pano_h), int(K)
    cell, w, dwx, dwy = contrast_votes(pm, W, H)
    n = cell.shape[0]
    s = np.ones(n)
    if signed and pol is not None:
        s = np.where(np.asarray(pol).reshape(-1)[:n] == 0, -1.0, 1.0)
    inside = cell >= 0
    if prior is None:
        img = np.zeros(W * H)
    else:
        img = np.array(prior, dtype=np.float64)
        if img.shape != (H, W):
            raise ValueError(f"the prior has {img.shape} cells, the image {H} x {W}")
        img = img.reshape(-1)
    np.add.at(img, cell[inside], (w * s[:, None])[inside])
    out = dict(image=img.reshape(H, W), J=float((img * img).sum()), dropped=int(np.count_nonzero(~inside & (w != 0))), grad=None)
    if D is None or cp is None:
        return out
    D = np.asarray(D, dtype=np.float64).reshape(n, 2, 6)
    cp = np.asarray(cp, dtype=np.int64).reshape(n)
    I4 = np.where(inside, img[np.where(inside, cell, 0)], 0.0)
    gx, gy = (I4 * dwx).sum(axis=1), (I4 * dwy).sum(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        ge = (2.0 * s)[:, None] * (gx[:, None] * D[:, 0, :] + gy[:, None] * D[:, 1, :])
    ge = np.where(np.isfinite(ge), ge, 0.0)
    live = (cp >= 0) & (cp <= K - 2)
    g = np.zeros((K, 3))
    np.add.at(g, cp[live], ge[live, :3])
    np.add.at(g, cp[live] + 1, ge[live, 3:])
    out["grad"] = g.reshape(-1)
    return out


def refine_contrast(J_and_grad, J_only, traj, fix_first_pose=True, max_iter=60, step_px=2.0, tol=1e-6, *, pano_w):
    """Polak-Ribiere+ conjugate-gradient ascent of the control poses of traj on a contrast J.  J_and_grad(traj) -> (J, g [3 K]) with g the gradient with
    respect to the increments of incremental_update, J_only(traj) -> J (the line search asks for nothing else).  With fix_first_pose the first control
    pose's three components of g are zeroed.  Per iteration: the direction d is scaled so that its largest component is 1; trial steps a d go through
    incremental_update, a starting at step_px 2 pi / pano_w (step_px pixels of azimuth on the panorama); a is halved up to 10 times until J rises
    strictly, and doubled after an accepted step, capped at 8 times the start; the loop restarts along g where d . g <= 0.  It stops when no halving
    helps, when the relative gain falls below tol, or after max_iter iterations.  pano_w is required: the first step is in pixels.  Returns (trajectory, [J at the start, J after every accepted step],
    evaluations of J)."""
    def grad_at(t):
        J, g = J_and_grad(t)
        g = np.array(g, dtype=np.float64).reshape(-1)
        if fix_first_pose:
            g[:3] = 0.0
        return float(J), g
    a0 = float(step_px) * 2.0 * np.pi / float(pano_w)
    a = a0
    J, g = grad_at(traj)
    evals, hist, d = 1, [J], g.copy()
    for _ in range(int(max_iter)):
        if float(d @ g) <= 0.0:
            d = g.copy()
        top = float(np.max(np.abs(d), initial=0.0))
        if not (top > 0.0 and np.isfinite(top)):
            break
        dn = d / top
        trial = Jt = None
        for _ in range(11):                                   # a, then up to 10 halvings
            cand = incremental_update(traj, a * dn, fix_first_pose)
            Jc = float(J_only(cand))
            evals += 1
            if Jc > J:
                trial, Jt = cand, Jc
                break
            a *= 0.5
        if trial is None:
            break
        gain = (Jt - J) / abs(Jt)
        traj = trial
        a = min(2.0 * a, 8.0 * a0)
        _, g_new = grad_at(traj)                               # (the next comparisons are made against J_only's value of this point: one form throughout)
        evals += 1
        hist.append(Jt)
        gg = float(g @ g)
        beta = max(0.0, float(g_new @ (g_new - g)) / gg) if gg > 0.0 else 0.0
        d = g_new + beta * d
        g = g_new
        J = Jt
        if gain < tol:
            break
    return traj, hist, evals


# ---- coarse to fine (numpy form of emba_seq_contrast_gradient_level, include/emba_hip.h): a level is the rule above on a coarser grid
CONTRAST_MAX_LEVEL = 8      # kContrastMaxLevel (emba_amd/csrc/contrast_rule.h)


def contrast_level(pm, D, pano_w, pano_h, level):
    """Level `level` of the smooth contrast: (pm_l, D_l, W_l, H_l) with W_l = pano_w >> level, H_l = pano_h >> level, pm_l = pm 2^-level and D_l = D 2^-level
    (exact scalings; D may be None) — contrast_gradient(pm_l, D_l, cp, pol, K, W_l, H_l) is then the rule of emba_seq_contrast_gradient_level.  Level 0
    returns pm and D as they are.  ValueError, as the library refuses: a level outside [0, CONTRAST_MAX_LEVEL], a panorama not divisible by 2^level, fewer
    than two rows left."""
    W, H, l = int(pano_w), int(pano_h), int(level)
    if not 0 <= l <= CONTRAST_MAX_LEVEL:
        raise ValueError(f"level {level}: levels are 0 ... {CONTRAST_MAX_LEVEL}")
    if W % (1 << l) or H % (1 << l):
        raise ValueError(f"level {l}: a panorama of {W} x {H} cells is not divisible by {1 << l}")
    if (H >> l) < 2:
        raise ValueError(f"level {l}: {H} rows of {1 << l} leave fewer than two")
    scale = 1.0 / (1 << l)
    pm = np.asarray(pm, dtype=np.float64)
    return pm * scale, (None if D is None else np.asarray(D, dtype=np.float64) * scale), W >> l, H >> l


def check_contrast_levels(levels, pano_w):
    """The schedule of a pyramid as a tuple of ints: strictly decreasing, ending at level 0, every level one the panorama's width is divisible by."""
    lv = tuple(int(l) for l in levels)
    if not lv or lv[-1] != 0:
        raise ValueError(f"contrast levels {lv}: the schedule must end at level 0, the panorama itself")
    for a, b in zip(lv, lv[1:]):
        if not a > b:
            raise ValueError(f"contrast levels {lv}: levels must be strictly decreasing, coarse to fine ({a} is followed by {b})")
    if lv[0] > CONTRAST_MAX_LEVEL:
        raise ValueError(f"contrast levels {lv}: levels are 0 ... {CONTRAST_MAX_LEVEL}")
    if int(pano_w) % (1 << lv[0]):
        raise ValueError(f"contrast levels {lv}: a panorama {int(pano_w)} cells wide is not divisible by {1 << lv[0]}")
    return lv


def refine_contrast_pyramid(J_and_grad_at, J_only_at, traj, levels, *, pano_w, **kw):
    """refine_contrast coarse to fine.  J_and_grad_at(level) and J_only_at(level) return the two callables of refine_contrast for that level's contrast;
    levels: strictly decreasing and ending at 0 (check_contrast_levels), e.g. (3, 2, 1, 0).  Each level runs refine_contrast with pano_w >> level — the
    first trial step is step_px of THAT level's cells — and hands its trajectory to the next finer one; **kw goes to every level (fix_first_pose,
    max_iter, step_px, tol).  Returns (trajectory, {level: [J at the level's start, J after every accepted step]}, evaluations of J over all levels).
    A level's J are not comparable with another level's: the histories stay apart."""
    lv = check_contrast_levels(levels, pano_w)
    hists, evals = {}, 0
    for l in lv:
        traj, hist, n = refine_contrast(J_and_grad_at(l), J_only_at(l), traj, pano_w=int(pano_w) >> l, **kw)
        hists[l] = hist
        evals += n
    return traj, hists, evals


def refine_contrast_levels(model, traj, beg, end, levels, *, pano_w, fix_first_pose=True, max_iter=60, prior_weight=None):
    """refine_contrast_pyramid over model.contrast_gradient(..., level=l) on the events [beg, end) of the model's resident sequence: (trajectory, J at
    level 0 before, J at level 0 after, evaluations over all levels — the one of J before included where the schedule does not start at level 0).
    prior_weight: None, or the weight of the model's priors — every call of every level then asks
    model.contrast_gradient(..., prior_weight=prior_weight), J before and after included, and every level of the schedule needs a prior."""
    lv = check_contrast_levels(levels, pano_w)
    kw = {} if prior_weight is None else dict(prior_weight=float(prior_weight))      # (none: the calls made before there were priors)

    def J_and_grad_at(l):
        def f(t):
            r = model.contrast_gradient(t, beg, end, level=l, **kw)
            return r["J"], r["grad"]
        return f

    def J_only_at(l):
        return lambda t: model.contrast_gradient(t, beg, end, want_grad=False, level=l, **kw)["J"]
    extra = 0 if lv[0] == 0 else 1
    J_before = float(J_only_at(0)(traj)) if extra else None
    out, hists, evals = refine_contrast_pyramid(J_and_grad_at, J_only_at, traj, lv, pano_w=pano_w, fix_first_pose=fix_first_pose, max_iter=int(max_iter))
    return out, (hists[0][0] if J_before is None else J_before), hists[0][-1], evals + extra


# ---- sensor views along the trajectory (numpy forms of emba_render_views and emba_seq_event_frames, include/emba_hip.h; the device forms are
# LEGM.render_views and LEGM.event_frames).  The sample and the tone are emba_amd/csrc/view_rule.h's view_sample and view_u8, operation for
# operation: given the same pm both forms give the same bits.  The event frames are integers.
def view_pm(lut, knots, t0_ns, dt_ns, frame_t_ns, W, H):
    """pm [F, S, 2] of every sensor pixel (S rows of the bearing LUT) at every frame time: the spline pose by so3.spline_evaluate, pm = project(R * bearing)
    with the equirectangular projection of synth.project_equirect on a panorama of W x H.  numpy's sin / atan2 / asin are not the device's: close to
    emba_render_views' pm_out, not bit-equal.  Raises ValueError where a frame time lies outside the knots (so3.spline_evaluate)."""
    from . import synth
    lut = np.asarray(lut, dtype=np.float64).reshape(-1, 3)
    knots = np.asarray(knots, dtype=np.float64).reshape(-1, 4)
    ts = np.asarray(frame_t_ns, dtype=np.int64).reshape(-1)
    pm = np.zeros((ts.size, lut.shape[0], 2))
    for f, t in enumerate(ts.tolist()):
        rb = lut @ synth._quat_to_R(so3.spline_evaluate(knots, int(t0_ns), int(dt_ns), t)).T
        pm[f, :, 0], pm[f, :, 1] = synth.project_equirect(int(W), int(H), rb)
    return pm


def render_views(plane, pm, fill=0.0, with_outside=False):
    """view_sample (view_rule.h) of plane [H, W] at every pm [..., 2]: ix = floor(pm_x), ax = pm_x - ix, iy, ay likewise; the columns ix, ix + 1 wrap modulo
    W; iy < 0 or iy + 1 > H - 1 (or a pm that is not finite, or |pm| >= 2^31) is outside and reads `fill`; otherwise
    (1 - ay) ((1 - ax) P[iy][ix] + ax P[iy][ix + 1]) + ay ((1 - ax) P[iy + 1][ix] + ax P[iy + 1][ix + 1]), in this order.  Returns the views, shaped
    pm.shape[:-1]; with_outside also the boolean mask of the outside pixels."""
    P = np.asarray(plane, dtype=np.float64)
    H, W = P.shape
    pm = np.asarray(pm, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(pm[..., 0]) < 2147483648.0) & (np.abs(pm[..., 1]) < 2147483648.0)
    x, y = np.where(ok, pm[..., 0], 0.0), np.where(ok, pm[..., 1], -1.0)
    fx, fy = np.floor(x), np.floor(y)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    inside = ok & (iy >= 0) & (iy + 1 <= H - 1)
    ax, ay = x - fx, y - fy
    c0 = ix % W
    c1 = np.where(c0 + 1 == W, 0, c0 + 1)
    r0 = np.where(inside, iy, 0)
    r1 = np.where(inside, iy + 1, 0)
    top = (1.0 - ax) * P[r0, c0] + ax * P[r0, c1]
    bot = (1.0 - ax) * P[r1, c0] + ax * P[r1, c1]
    views = np.where(inside, (1.0 - ay) * top + ay * bot, float(fill))
    return (views, ~inside) if with_outside else views


def view_u8(views, lo, hi, outside=None):
    """view_u8 (view_rule.h): sat(rint(scale (v - lo))) with scale = 255 / (hi - lo), or 1 where hi == lo — the arithmetic of normalize_robust with the
    caller's limits; a NaN is 0, and so is every pixel of the mask `outside`."""
    v = np.asarray(views, dtype=np.float64)
    scale = 255.0 / (float(hi) - float(lo)) if hi != lo else 1.0
    with np.errstate(invalid="ignore"):
        r = np.rint(scale * (v - float(lo)))
        u8 = np.where(r > 0.0, np.minimum(r, 255.0), 0.0).astype(np.uint8)
    return u8 if outside is None else np.where(outside, np.uint8(0), u8)


def event_frames(x, y, pol, t, edges, sw, sh, signed_polarity=True):
    """The rule of emba_seq_event_frames: F = len(edges) - 1 frames int32 [F, sh, sw]; event k belongs to frame f when edges[f] <= t[k] < edges[f + 1] and
    adds +1 to its pixel there, or -1 for polarity 0 with signed_polarity.  Returns (frames, before, after): the events before edges[0] and at or after
    edges[F].  Every event counts (no batches).  The edges must be strictly increasing."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1)
    if edges.size < 1 or (np.diff(edges) <= 0).any():
        raise ValueError("the edges must be strictly increasing (F + 1 of them)")
    F, sw, sh = edges.size - 1, int(sw), int(sh)
    t = np.asarray(t, dtype=np.int64).reshape(-1)
    f = np.searchsorted(edges, t, side="right") - 1
    keep = (f >= 0) & (f < F)
    cell = (f[keep] * sh + np.asarray(y, dtype=np.int64).reshape(-1)[keep]) * sw + np.asarray(x, dtype=np.int64).reshape(-1)[keep]
    w = np.where(np.asarray(pol).reshape(-1)[keep] == 0, -1.0, 1.0) if signed_polarity else np.ones(cell.size)
    frames = np.bincount(cell, weights=w, minlength=F * sh * sw).astype(np.int32).reshape(F, sh, sw)      # (sums of +-1: exact in a double)
    return frames, int((f < 0).sum()), int((f >= F).sum())


# ---- the mosaic of intensity frames (numpy forms of emba_mosaic_frames, emba_mosaic_get and emba_mosaic_map, include/emba_hip.h; the device forms are
# LEGM.mosaic_frames, LEGM.mosaic and LEGM.mosaic_map).  The rules are emba_amd/csrc/mosaic_rule.h's, operation for operation: given the same
# pm the sums are the same integers, given the same sums the mean has the same bits, given the same L the gradients have the same bits.  view_pm above
# gives numpy's own pm.
MOSAIC_MAX_VOTES = 1 << 36               # kMosaicMaxVotes: the frame pixels accumulated stay below this, so that both sums convert to double exactly


def mosaic_votes(frames_u8, pm, pano_w, pano_h, skip_zero=False):
    """The votes of the frame pixels frames_u8 [F, S] (any shape of F * S bytes) projected to pm [F, S, 2]: every pixel votes through pano_votes, cell c gets
    w into sum_w[c] and w * v into sum_v[c].  With skip_zero a pixel whose byte is 0 casts no vote and is counted.  Returns (sum_w uint64 [pano_h, pano_w],
    sum_v likewise, dropped, skipped): dropped the non-zero weights whose row lies outside the panorama, as python ints."""
    W, H = int(pano_w), int(pano_h)
    v = np.asarray(frames_u8, dtype=np.uint8).reshape(-1).astype(np.int64)
    if v.size >= MOSAIC_MAX_VOTES:
        raise ValueError(f"{v.size} frame pixels: the sums are exact below {MOSAIC_MAX_VOTES} votes")
    cell, w = pano_votes(pm, W, H)
    if cell.shape[0] != v.size:
        raise ValueError(f"pm has {cell.shape[0]} rows, the frames have {v.size} pixels")
    votes = (v != 0) if skip_zero else np.ones(v.size, dtype=bool)
    w = w * votes[:, None]
    inside = cell >= 0
    # (sums of integers below 2^53: exact in the doubles bincount adds)
    sum_w = np.bincount(cell[inside], weights=w[inside].astype(np.float64), minlength=W * H).astype(np.uint64).reshape(H, W)
    sum_v = np.bincount(cell[inside], weights=(w * v[:, None])[inside].astype(np.float64), minlength=W * H).astype(np.uint64).reshape(H, W)
    return sum_w, sum_v, int(np.count_nonzero(~inside & (w != 0))), int(np.count_nonzero(~votes))


def mosaic_mean(sum_w, sum_v, min_weight=256, fill=0.0):
    """mosaic_mean (mosaic_rule.h): covered = sum_w >= min_weight (min_weight >= 1); mean = double(sum_v) / double(sum_w) where covered, else `fill`.
    Returns (mean float64, covered bool)."""
    if int(min_weight) < 1:
        raise ValueError("min_weight is 1 at the least")
    sum_w, sum_v = np.asarray(sum_w, dtype=np.uint64), np.asarray(sum_v, dtype=np.uint64)
    covered = sum_w >= np.uint64(min_weight)
    mean = np.where(covered, sum_v.astype(np.float64) / np.where(covered, sum_w, np.uint64(1)).astype(np.float64), float(fill))
    return mean, covered


def mosaic_log(mean, covered, lo=0.0, hi=1.0, eps=1.0 / 255.0, take_log=True):
    """mosaic_log (mosaic_rule.h): I = lo + mean * (hi - lo) / 255 in this order, the inverse of view_u8's tone; L = I without take_log, else log(I + eps),
    and a cell whose I + eps is not positive becomes uncovered.  Returns (L float64, 0 where uncovered; covered bool)."""
    lo, hi, eps = float(lo), float(hi), float(eps)
    if not (np.isfinite(lo) and np.isfinite(hi) and np.isfinite(eps) and hi > lo):
        raise ValueError("lo, hi, eps are finite and hi > lo")
    covered = np.asarray(covered).astype(bool)
    inten = lo + np.asarray(mean, dtype=np.float64) * (hi - lo) / 255.0
    if not take_log:
        return np.where(covered, inten, 0.0), covered
    a = inten + eps
    with np.errstate(invalid="ignore"):
        covered = covered & (a > 0.0)
    return np.where(covered, np.log(np.where(covered, a, 1.0)), 0.0), covered


def gradient_from_plane(L, covered):
    """mosaic_gradient (mosaic_rule.h): backward differences of the plane L [H, W] with holes — Gx[i][j] = L[i][j] - L[i][(j - 1) mod W] where both cells
    are covered, Gy[i][j] = L[i][j] - L[i - 1][j] where both are covered and i >= 1, 0 elsewhere: the field whose divergence in reconstruct_intensity is the
    5-point operator.  Returns (Gx, Gy)."""
    L = np.asarray(L, dtype=np.float64)
    cov = np.asarray(covered).astype(bool)
    Gx = np.where(cov & np.roll(cov, 1, axis=1), L - np.roll(L, 1, axis=1), 0.0)
    Gy = np.zeros_like(L)
    Gy[1:] = np.where(cov[1:] & cov[:-1], L[1:] - L[:-1], 0.0)
    return Gx, Gy


# ---- the event simulator (numpy form of emba_simulate_events, include/emba_hip.h; the device form is LEGM.simulate_events).  The rule is
# emba_amd/csrc/sim_rule.h's sim_frame / sim_step, operation for operation: given the same samples both forms give the same events in the same order.
SIM_MAX_PER_STEP = 255
SIM_MAX_SPAN_NS = 1 << 52


def simulate_events(views, outside, step_t_ns, sensor_w, c_on, c_off=None, max_per_step=255):
    """The events of the samples views [F + 1, S] (S = sensor_h * sensor_w, any shape that reshapes to it) with the mask outside [F + 1, S] at the step times
    step_t_ns [F + 1], strictly increasing over less than 2^52 ns.  Every pixel s, over f = 0 ... F: V_f outside disarms it; V_f inside and the pixel not
    armed: ref = V_f, armed, no event; V_f inside and armed: prev = V_{f-1}, cur = V_f, d = step_t[f] - step_t[f-1], and while |cur - ref| >= C (C = c_on,
    sgn = +1 where cur - ref > 0, else C = c_off, sgn = -1), at most max_per_step times: ref = ref + sgn C; frac = (ref - prev) / (cur - prev), 0 where it
    is not >= 0, 1 where it is > 1; off = int64(frac * float(d)) truncated, at most d - 1; the event (x = s % sensor_w, y = s // sensor_w, polarity = sgn > 0,
    t = step_t[f-1] + off).  What the cap leaves over is carried in ref.  Order: ascending t, among equal t ascending s, among those the order of emission.
    Returns (EventPacket, stats uint64 [4]): events, positive events, (pixel, step) pairs where the condition still held after max_per_step events,
    (pixel, frame) pairs outside."""
    ts = np.asarray(step_t_ns, dtype=np.int64).reshape(-1)
    F = ts.size - 1
    if F < 1 or (np.diff(ts) <= 0).any() or int(ts[-1]) - int(ts[0]) >= SIM_MAX_SPAN_NS:
        raise ValueError("the step times must be strictly increasing over less than 2^52 ns (F + 1 of them, F >= 1)")
    c_on = float(c_on)
    c_off = c_on if c_off is None else float(c_off)
    if not (np.isfinite(c_on) and c_on > 0.0 and np.isfinite(c_off) and c_off > 0.0):
        raise ValueError("the thresholds must be positive and finite")
    max_per_step, sw = int(max_per_step), int(sensor_w)
    if not 1 <= max_per_step <= SIM_MAX_PER_STEP:
        raise ValueError(f"max_per_step must be 1 ... {SIM_MAX_PER_STEP}")
    V = np.asarray(views, dtype=np.float64).reshape(F + 1, -1)
    out = np.asarray(outside, dtype=bool).reshape(F + 1, -1)
    if out.shape != V.shape or V.shape[1] % sw:
        raise ValueError("views and outside must both be [F + 1, sensor_h * sensor_w]")
    armed = ~out[0]
    ref = np.where(armed, V[0], 0.0)
    n_cap = 0
    ev_s, ev_pol, ev_t = [], [], []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for f in range(1, F + 1):
            inside = ~out[f]
            idx = np.flatnonzero(inside & armed)
            t_prev, d = int(ts[f - 1]), int(ts[f] - ts[f - 1])
            r, p, c = ref[idx], V[f - 1][idx], V[f][idx]
            s_f, k_f, pol_f, t_f = [], [], [], []
            k = 0
            while idx.size:
                diff = c - r
                up = diff > 0.0
                C = np.where(up, c_on, c_off)
                go = np.abs(diff) >= C
                idx, r, p, c, up, C = idx[go], r[go], p[go], c[go], up[go], C[go]
                if k == max_per_step:
                    n_cap += idx.size
                    break
                if not idx.size:
                    break
                r = r + np.where(up, 1.0, -1.0) * C
                frac = (r - p) / (c - p)
                frac = np.where(frac >= 0.0, frac, 0.0)
                frac = np.where(frac > 1.0, 1.0, frac)
                off = np.minimum((frac * float(d)).astype(np.int64), d - 1)
                ref[idx] = r
                s_f.append(idx); k_f.append(np.full(idx.size, k)); pol_f.append(up); t_f.append(t_prev + off)
                k += 1
            if s_f:
                s_f, k_f, pol_f, t_f = np.concatenate(s_f), np.concatenate(k_f), np.concatenate(pol_f), np.concatenate(t_f)
                order = np.lexsort((k_f, s_f, t_f))      # by t, then pixel, then emission
                ev_s.append(s_f[order]); ev_pol.append(pol_f[order]); ev_t.append(t_f[order])
            fresh = inside & ~armed
            ref[fresh] = V[f][fresh]
            armed = inside
    s_all = np.concatenate(ev_s) if ev_s else np.zeros(0, np.int64)
    pol = (np.concatenate(ev_pol) if ev_pol else np.zeros(0, bool)).astype(np.uint8)
    t = np.concatenate(ev_t).astype(np.int64) if ev_t else np.zeros(0, np.int64)
    stats = np.array([t.size, int(pol.sum()), n_cap, int(out.sum())], dtype=np.uint64)
    return EventPacket((s_all % sw).astype(np.uint16), (s_all // sw).astype(np.uint16), pol, t), stats


def simulate_from_plane(plane, lut, knots, t0_ns, dt_ns, step_t_ns, sensor, c_on, c_off=None, max_per_step=255):
    """A recording without the device: the samples of `plane` [H, W] at the step times along the spline (view_pm, then render_views), then simulate_events.
    sensor = (sensor_w, sensor_h).  numpy's pm is close to the device's, not bit-equal: so are the samples, and an event near a threshold may differ."""
    P = np.asarray(plane, dtype=np.float64)
    pm = view_pm(lut, knots, t0_ns, dt_ns, step_t_ns, P.shape[1], P.shape[0])
    views, outside = render_views(P, pm, with_outside=True)
    return simulate_events(views, outside, step_t_ns, int(sensor[0]), c_on, c_off, max_per_step)


# ---- intensity frames aligned to a panorama plane (numpy forms of emba_frames_align_eval and emba_frames_align, include/emba_hip.h; the device forms are
# LEGM.align_frames_eval and LEGM.align_frames).  The rule is emba_amd/csrc/align_rule.h's, operation for operation where bits are promised:
# given the same pm, the sample, its gradient, the classes and the residual have the same bits.  rb and J23 are numpy's own.
ALIGN_CONVERGED, ALIGN_STALLED, ALIGN_ITERATIONS, ALIGN_DEGENERATE = 1, 2, 3, 4      # EMBA_ALIGN_*
ALIGN_STATUS_NAMES = {1: "converged", 2: "stalled", 3: "iterations", 4: "degenerate"}
ALIGN_USED, ALIGN_OUTSIDE, ALIGN_MASKED, ALIGN_SKIPPED = 0, 1, 2, 3                  # the classes of a pixel, in the order of counts
ALIGN_DEFAULTS = dict(max_iters=30, lambda0=1e-3, lambda_up=10.0, lambda_down=10.0, lambda_min=1e-9, lambda_max=1e6, tol_rot=1e-6, min_pixels=16, huber_k=0.0)


def align_settings(**kw):
    """ALIGN_DEFAULTS with the given members replaced; the refusals of emba_frames_align's settings as ValueError."""
    unknown = set(kw) - set(ALIGN_DEFAULTS)
    if unknown:
        raise ValueError(f"unknown settings {sorted(unknown)}")
    s = dict(ALIGN_DEFAULTS, **kw)
    ok = (int(s["max_iters"]) >= 0 and np.isfinite(s["lambda_up"]) and np.isfinite(s["lambda_down"]) and s["lambda_up"] > 1.0 and s["lambda_down"] > 1.0
          and np.isfinite(s["lambda0"]) and s["lambda0"] > 0.0 and 0.0 <= s["lambda_min"] <= s["lambda_max"] and s["lambda_max"] > 0.0 and s["tol_rot"] >= 0.0
          and int(s["min_pixels"]) >= 3 and not np.isnan(s["huber_k"]))
    if not ok:
        raise ValueError(f"settings out of range: {s}")
    return s


def _align_cell(shape, pm):
    """view_sample's cell of every pm [..., 2] on a plane of `shape`: (inside, r0, r1, c0, c1, ax, ay); the rows of an outside pixel are 0."""
    H, W = shape
    pm = np.asarray(pm, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(pm[..., 0]) < 2147483648.0) & (np.abs(pm[..., 1]) < 2147483648.0)
    x, y = np.where(ok, pm[..., 0], 0.0), np.where(ok, pm[..., 1], -1.0)
    fx, fy = np.floor(x), np.floor(y)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    inside = ok & (iy >= 0) & (iy + 1 <= H - 1)
    c0 = ix % W
    c1 = np.where(c0 + 1 == W, 0, c0 + 1)
    return inside, np.where(inside, iy, 0), np.where(inside, iy + 1, 0), c0, c1, x - fx, y - fy


def align_sample(plane, pm):
    """align_sample (align_rule.h) of plane [H, W] at every pm [..., 2]: (val, gx, gy, outside).  The cell and the outside test are render_views'; val is its
    value, gx = (1 - ay) (P[iy][c1] - P[iy][c0]) + ay (P[iy+1][c1] - P[iy+1][c0]), gy = (1 - ax) (P[iy+1][c0] - P[iy][c0]) + ax (P[iy+1][c1] - P[iy][c1]),
    in this order.  All three are 0 where the pixel is outside."""
    P = np.asarray(plane, dtype=np.float64)
    inside, r0, r1, c0, c1, ax, ay = _align_cell(P.shape, pm)
    p00, p01, p10, p11 = P[r0, c0], P[r0, c1], P[r1, c0], P[r1, c1]
    top = (1.0 - ax) * p00 + ax * p01
    bot = (1.0 - ax) * p10 + ax * p11
    val = (1.0 - ay) * top + ay * bot
    gx = (1.0 - ay) * (p01 - p00) + ay * (p11 - p10)
    gy = (1.0 - ax) * (p10 - p00) + ax * (p11 - p01)
    return np.where(inside, val, 0.0), np.where(inside, gx, 0.0), np.where(inside, gy, 0.0), ~inside


def align_warp(lut, q, W, H):
    """numpy's own warp of one frame with the rotation q (xyzw): rb = R(q) lut [S, 3], pm [S, 2] by synth.project_equirect and J23 [S, 2, 3] = d pm / d delta
    for the left perturbation R <- exp(delta) R (the equirectangular projection's Jacobian times -[rb]x)."""
    from . import synth
    lut = np.asarray(lut, dtype=np.float64).reshape(-1, 3)
    rb = lut @ synth._quat_to_R(np.asarray(q, dtype=np.float64)).T
    px, py = synth.project_equirect(int(W), int(H), rb)
    x, y, z = rb[:, 0], rb[:, 1], rb[:, 2]
    fx, fy = W / (2.0 * np.pi), H / np.pi
    d2 = x * x + z * z
    rho2 = d2 + y * y
    s = fy / (np.sqrt(d2) * rho2)
    zero = np.zeros_like(x)
    Jp = np.stack([np.stack([fx * z / d2, zero, -fx * x / d2], axis=1), np.stack([-s * x * y, s * d2, -s * y * z], axis=1)], axis=1)      # [S, 2, 3]
    M = np.stack([np.stack([zero, z, -y], axis=1), np.stack([-z, zero, x], axis=1), np.stack([y, -x, zero], axis=1)], axis=1)               # -[rb]x
    return rb, np.stack([px, py], axis=1), Jp @ M


def align_huber(r, huber_k):
    """(w, rho) of the residuals r: huber_k <= 0 quadratic; else w = 1, rho = r^2 for |r| <= k and w = k / |r|, rho = 2 k |r| - k^2 beyond."""
    r = np.asarray(r, dtype=np.float64)
    k = float(huber_k)
    a = np.abs(r)
    if not k > 0.0:
        return np.ones_like(r), r * r
    far = a > k
    return np.where(far, k / np.where(far, a, 1.0), 1.0), np.where(far, 2.0 * k * a - k * k, r * r)


def align_terms(frame_u8, pm, lut, q, plane, valid=None, lo=0.0, hi=255.0, skip_zero=False, huber_k=0.0):
    """The terms of one frame's pixels (align_pixel, align_rule.h) from a given pm [S, 2] (the device's pm_out, or align_warp's) and numpy's own J23 of q: a
    dict of cls int [S] (ALIGN_USED / OUTSIDE / MASKED / SKIPPED, in this precedence), r [S] (val - I with I = lo + v (hi - lo) / 255; 0 where the pixel is
    not used), w, rho [S] and g [S, 3] = gx J23[0,:] + gy J23[1,:]."""
    P = np.asarray(plane, dtype=np.float64)
    H, W = P.shape
    v = np.asarray(frame_u8, dtype=np.uint8).reshape(-1)
    pm = np.asarray(pm, dtype=np.float64).reshape(-1, 2)
    if pm.shape[0] != v.size:
        raise ValueError(f"pm has {pm.shape[0]} rows, the frame has {v.size} pixels")
    val, gx, gy, outside = align_sample(P, pm)
    cls = np.full(v.size, ALIGN_USED, dtype=np.int64)
    if skip_zero:
        cls[v == 0] = ALIGN_SKIPPED
    if valid is not None:
        ok = np.asarray(valid).astype(bool)
        _, r0, r1, c0, c1, _, _ = _align_cell(P.shape, pm)
        cls[~(ok[r0, c0] & ok[r0, c1] & ok[r1, c0] & ok[r1, c1])] = ALIGN_MASKED
    cls[outside] = ALIGN_OUTSIDE
    used = cls == ALIGN_USED
    inten = float(lo) + v.astype(np.float64) * (float(hi) - float(lo)) / 255.0
    r = np.where(used, val - inten, 0.0)
    w, rho = align_huber(r, huber_k)
    J23 = align_warp(lut, q, W, H)[2]
    g = gx[:, None] * J23[:, 0, :] + gy[:, None] * J23[:, 1, :]
    return dict(cls=cls, r=r, w=np.where(used, w, 0.0), rho=np.where(used, rho, 0.0), g=np.where(used[:, None], g, 0.0))


def align_sum_terms(terms):
    """The ten terms of every pixel [S, 10] (H 00 01 02 11 12 22, b 0 1 2, rho), zero where the pixel is not used."""
    g, w, r = terms["g"], terms["w"], terms["r"]
    wg = w[:, None] * g
    return np.stack([wg[:, 0] * g[:, 0], wg[:, 0] * g[:, 1], wg[:, 0] * g[:, 2], wg[:, 1] * g[:, 1], wg[:, 1] * g[:, 2], wg[:, 2] * g[:, 2],
                     wg[:, 0] * r, wg[:, 1] * r, wg[:, 2] * r, terms["rho"]], axis=1)


def align_sums(terms, with_scale=False):
    """The ten sums and the four counts of one frame's terms: (sums float64 [10], counts int64 [4]: used, outside, masked, skipped), accumulated in
    np.longdouble and returned as doubles.  with_scale also sum |term| per sum, what a bound on a sum's rounding error is relative to."""
    t = align_sum_terms(terms)
    sums = t.astype(np.longdouble).sum(axis=0).astype(np.float64)
    counts = np.bincount(terms["cls"], minlength=4).astype(np.int64)
    return (sums, counts, np.abs(t).astype(np.longdouble).sum(axis=0).astype(np.float64)) if with_scale else (sums, counts)


def align_step(Hm, b, lam):
    """align_solve (align_rule.h): delta [3] of (H + lam diag H) delta = -b by a Cholesky, H [3, 3] symmetric (or its six entries 00 01 02 11 12 22); None where a
    pivot is not positive."""
    Hm = np.asarray(Hm, dtype=np.float64)
    if Hm.size == 6:
        h = Hm.reshape(6)
        Hm = np.array([[h[0], h[1], h[2]], [h[1], h[3], h[4]], [h[2], h[4], h[5]]])
    A = Hm + float(lam) * np.diag(np.diag(Hm))
    L = np.zeros((3, 3))
    for j in range(3):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0.0:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 3):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(3)
    rhs = -np.asarray(b, dtype=np.float64).reshape(3)
    for i in range(3):
        y[i] = (rhs[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(3)
    for i in (2, 1, 0):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x if np.isfinite(x).all() else None


def align_frames(frames_u8, q_xyzw, lut, plane, valid=None, lo=0.0, hi=255.0, skip_zero=False, **settings):
    """The loop of emba_frames_align in numpy, with numpy's own pm: per frame (frames_u8 [F, S], q_xyzw [F, 4]) the Levenberg-Marquardt iteration of
    align_step (align_rule.h) — solve, trial q' = normalise(exp(delta) q), accepted when n' >= min_pixels and cost' / n' < cost / n, lambda down on accept and
    up on reject; a frame ends converged (|delta| < tol_rot on an accepted step), stalled (lambda > lambda_max), out of iterations or degenerate.  A dict of q
    [F, 4], sums [F, 10], counts [F, 4], status, iters, cost0, n0 [F]."""
    s = align_settings(**settings)
    P = np.asarray(plane, dtype=np.float64)
    H, W = P.shape
    q_in = np.asarray(q_xyzw, dtype=np.float64).reshape(-1, 4)
    F = q_in.shape[0]
    frames = np.asarray(frames_u8, dtype=np.uint8).reshape(F, -1)

    def evaluate(f, q):
        return align_sums(align_terms(frames[f], align_warp(lut, q, W, H)[1], lut, q, P, valid, lo, hi, skip_zero, s["huber_k"]))

    out = dict(q=q_in.copy(), sums=np.zeros((F, 10)), counts=np.zeros((F, 4), np.int64), status=np.zeros(F, np.int32), iters=np.zeros(F, np.int32),
               cost0=np.zeros(F), n0=np.zeros(F, np.int64))
    for f in range(F):
        q = q_in[f].copy()
        sums, counts = evaluate(f, q)
        out["cost0"][f], out["n0"][f] = sums[9], counts[0]
        lam, iters = float(s["lambda0"]), 0
        while True:
            delta = align_step(sums[:6], sums[6:9], lam) if counts[0] >= s["min_pixels"] else None
            if delta is None:
                status = ALIGN_DEGENERATE
                break
            if iters >= s["max_iters"]:
                status = ALIGN_ITERATIONS
                break
            trial = so3.mul(so3.exp(delta), q)
            tsums, tcounts = evaluate(f, trial)
            iters += 1
            if tcounts[0] >= s["min_pixels"] and tsums[9] / tcounts[0] < sums[9] / counts[0]:
                q, sums, counts = trial, tsums, tcounts
                lam = max(lam / s["lambda_down"], s["lambda_min"])
                if np.linalg.norm(delta) < s["tol_rot"]:
                    status = ALIGN_CONVERGED
                    break
            else:
                lam *= s["lambda_up"]
                if lam > s["lambda_max"]:
                    status = ALIGN_STALLED
                    break
        out["q"][f], out["sums"][f], out["counts"][f], out["status"][f], out["iters"][f] = q, sums, counts, status, iters
    return out


# ---- per-frame exposure (numpy forms of emba_frames_exposure_eval, emba_frames_exposure_align and emba_mosaic_frames_exposure, include/emba_hip.h; the
# device forms are LEGM.exposure_eval, LEGM.align_frames_exposure and LEGM.mosaic_frames_exposure).  The rule is
# emba_amd/csrc/exposure_rule.h's: frame f carries (q_f, a_f, b_f), its compensated intensity is a_f * I0 + b_f.  Given the same pm, the classes are the same
# and the residuals have the same bits; given the same pm, io.mosaic_votes of exposure_bytes gives the same integer sums.
EXPOSURE_GAIN, EXPOSURE_BIAS = 1, 2                                  # EMBA_EXPOSURE_*: the bits of `estimate`
EXPOSURE_SUMS, EXPOSURE_RHS, EXPOSURE_COST = 21, 15, 20
EXPOSURE_SHARED = (0, 1, 2, 5, 6, 9, 15, 16, 17, 20)                 # where align_sums' ten lie among the 21 (exposure_shared_index)
EXPOSURE_COLLINEAR = 1e-9                                            # kExposureCollinear
EXPOSURE_BOUNDS = dict(gain_min=0.25, gain_max=4.0)


def exposure_h_index(i, j):
    """The place of H[i][j], i <= j, among the 15 entries of the upper triangle in row-major order over (delta0, delta1, delta2, a, b)."""
    return i * 5 - i * (i - 1) // 2 + (j - i)


def exposure_bounds(gain_min=None, gain_max=None):
    """(gain_min, gain_max), EXPOSURE_BOUNDS where None; the refusal of emba_frames_exposure_align's bounds as ValueError."""
    lo = float(EXPOSURE_BOUNDS["gain_min"] if gain_min is None else gain_min)
    hi = float(EXPOSURE_BOUNDS["gain_max"] if gain_max is None else gain_max)
    if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo <= 1.0 <= hi):
        raise ValueError(f"gain_min = {lo}, gain_max = {hi}: finite, 0 < gain_min <= 1 <= gain_max")
    return lo, hi


def exposure_check(gain, bias, F):
    """gain, bias as float64 [F]; the refusals of the entry points as ValueError: not finite, a gain <= 0."""
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(gain, dtype=np.float64), (F,)))
    b = np.ascontiguousarray(np.broadcast_to(np.asarray(bias, dtype=np.float64), (F,)))
    if not (np.isfinite(a).all() and np.isfinite(b).all() and (a > 0.0).all()):
        raise ValueError("every gain is finite and positive, every bias finite")
    return a, b


def exposure_terms(frame_u8, pm, lut, q, plane, gain=1.0, bias=0.0, valid=None, lo=0.0, hi=255.0, skip_zero=False, huber_k=0.0):
    """The terms of one frame's pixels (exposure_pixel, exposure_rule.h) from a given pm [S, 2] and numpy's own J23 of q: align_terms' dict — cls in
    align_terms' precedence (skipped tests the raw byte), r = val - (gain * I0 + bias) with I0 = lo + v (hi - lo) / 255 (multiply, then add), w, rho, g —
    and I0 [S] (0 where the pixel is not used).  The Jacobian row of r is (g, -I0, -1)."""
    P = np.asarray(plane, dtype=np.float64)
    H, W = P.shape
    v = np.asarray(frame_u8, dtype=np.uint8).reshape(-1)
    pm = np.asarray(pm, dtype=np.float64).reshape(-1, 2)
    if pm.shape[0] != v.size:
        raise ValueError(f"pm has {pm.shape[0]} rows, the frame has {v.size} pixels")
    val, gx, gy, outside = align_sample(P, pm)
    cls = np.full(v.size, ALIGN_USED, dtype=np.int64)
    if skip_zero:
        cls[v == 0] = ALIGN_SKIPPED
    if valid is not None:
        ok = np.asarray(valid).astype(bool)
        _, r0, r1, c0, c1, _, _ = _align_cell(P.shape, pm)
        cls[~(ok[r0, c0] & ok[r0, c1] & ok[r1, c0] & ok[r1, c1])] = ALIGN_MASKED
    cls[outside] = ALIGN_OUTSIDE
    used = cls == ALIGN_USED
    I0 = float(lo) + v.astype(np.float64) * (float(hi) - float(lo)) / 255.0
    scaled = float(gain) * I0
    r = np.where(used, val - (scaled + float(bias)), 0.0)
    w, rho = align_huber(r, huber_k)
    J23 = align_warp(lut, q, W, H)[2]
    g = gx[:, None] * J23[:, 0, :] + gy[:, None] * J23[:, 1, :]
    return dict(cls=cls, r=r, w=np.where(used, w, 0.0), rho=np.where(used, rho, 0.0), g=np.where(used[:, None], g, 0.0), I0=np.where(used, I0, 0.0))


def exposure_sum_terms(terms):
    """The 21 terms of every pixel [S, 21]: w J^T J's upper triangle in row-major order, w J^T r, rho, with J = (g, -I0, -1); zero where the pixel is not
    used.  The columns EXPOSURE_SHARED are align_sum_terms', by the same operations."""
    g, w, r = terms["g"], terms["w"], terms["r"]
    J = np.concatenate([g, -terms["I0"][:, None], np.where(terms["cls"] == ALIGN_USED, -1.0, 0.0)[:, None]], axis=1)
    wJ = w[:, None] * J
    cols = [wJ[:, i] * J[:, j] for i in range(5) for j in range(i, 5)] + [wJ[:, i] * r for i in range(5)] + [terms["rho"]]
    return np.stack(cols, axis=1)


def exposure_sums(terms, with_scale=False):
    """The 21 sums and the four counts of one frame's terms, as align_sums gives its ten: (sums float64 [21], counts int64 [4]) and, with_scale, sum |term|
    per sum."""
    t = exposure_sum_terms(terms)
    sums = t.astype(np.longdouble).sum(axis=0).astype(np.float64)
    counts = np.bincount(terms["cls"], minlength=4).astype(np.int64)
    return (sums, counts, np.abs(t).astype(np.longdouble).sum(axis=0).astype(np.float64)) if with_scale else (sums, counts)


def exposure_collinear(sums):
    """exposure_collinear (exposure_rule.h): the undamped pivot of the bias behind the gain, H44 - H34^2 / H33, is at most EXPOSURE_COLLINEAR of H44."""
    h33, h34, h44 = (float(sums[k]) for k in (12, 13, 14))
    if not (h33 > 0.0 and h44 > 0.0):
        return True
    return not (h44 - h34 * h34 / h33 > EXPOSURE_COLLINEAR * h44)


def exposure_step(sums, lam, estimate):
    """exposure_solve (exposure_rule.h): x [5] = (delta, x_a, x_b) of (H + lam diag H) x = -b on the active rows of the 21 sums by a Cholesky, zero where a
    parameter is not estimated (estimate: EXPOSURE_GAIN | EXPOSURE_BIAS).  estimate = 0 is align_step itself.  None where the frame is degenerate: a pivot
    is not positive, or gain and bias are both estimated and their columns collinear."""
    sums = np.asarray(sums, dtype=np.float64).reshape(EXPOSURE_SUMS)
    estimate = int(estimate)
    if not 0 <= estimate <= 3:
        raise ValueError("estimate is a mask of EXPOSURE_GAIN and EXPOSURE_BIAS")
    x = np.zeros(5)
    if estimate == 0:
        ten = sums[list(EXPOSURE_SHARED)]
        delta = align_step(ten[:6], ten[6:9], lam)
        if delta is None:
            return None
        x[:3] = delta
        return x
    if estimate == 3 and exposure_collinear(sums):
        return None
    idx = [0, 1, 2] + ([3] if estimate & EXPOSURE_GAIN else []) + ([4] if estimate & EXPOSURE_BIAS else [])
    n = len(idx)
    A = np.array([[sums[exposure_h_index(min(i, j), max(i, j))] for j in idx] for i in idx])
    A = A + float(lam) * np.diag(np.diag(A))
    L = np.zeros((n, n))
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0.0:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    rhs = -sums[[EXPOSURE_RHS + i for i in idx]]
    y = np.zeros(n)
    for i in range(n):
        y[i] = (rhs[i] - L[i, :i] @ y[:i]) / L[i, i]
    z = np.zeros(n)
    for i in range(n - 1, -1, -1):
        z[i] = (y[i] - L[i + 1:, i] @ z[i + 1:]) / L[i, i]
    if not np.isfinite(z).all():
        return None
    x[idx] = z
    return x


def align_frames_exposure(frames_u8, q_xyzw, lut, plane, gain=1.0, bias=0.0, estimate=3, valid=None, lo=0.0, hi=255.0, skip_zero=False, gain_min=None,
                          gain_max=None, **settings):
    """The loop of emba_frames_exposure_align in numpy, with numpy's own pm: align_frames with (a, b) beside q — the trial is q' = normalise(exp(delta) q),
    a' = a + x_a, b' = b + x_b; accepted as align_frames accepts, and rejected when its estimated gain lies outside [gain_min, gain_max]; converged tests
    |delta| < tol_rot.  A dict of q [F, 4], gain, bias [F], sums [F, 21], counts [F, 4], status, iters, cost0, n0 [F]."""
    s = align_settings(**settings)
    g_lo, g_hi = exposure_bounds(gain_min, gain_max)
    estimate = int(estimate)
    if not 0 <= estimate <= 3:
        raise ValueError("estimate is a mask of EXPOSURE_GAIN and EXPOSURE_BIAS")
    P = np.asarray(plane, dtype=np.float64)
    H, W = P.shape
    q_in = np.asarray(q_xyzw, dtype=np.float64).reshape(-1, 4)
    F = q_in.shape[0]
    frames = np.asarray(frames_u8, dtype=np.uint8).reshape(F, -1)
    a_in, b_in = exposure_check(gain, bias, F)

    def evaluate(f, q, a, b):
        return exposure_sums(exposure_terms(frames[f], align_warp(lut, q, W, H)[1], lut, q, P, a, b, valid, lo, hi, skip_zero, s["huber_k"]))

    out = dict(q=q_in.copy(), gain=a_in.copy(), bias=b_in.copy(), sums=np.zeros((F, EXPOSURE_SUMS)), counts=np.zeros((F, 4), np.int64),
               status=np.zeros(F, np.int32), iters=np.zeros(F, np.int32), cost0=np.zeros(F), n0=np.zeros(F, np.int64))
    for f in range(F):
        q, a, b = q_in[f].copy(), float(a_in[f]), float(b_in[f])
        sums, counts = evaluate(f, q, a, b)
        out["cost0"][f], out["n0"][f] = sums[EXPOSURE_COST], counts[0]
        lam, iters = float(s["lambda0"]), 0
        while True:
            x = exposure_step(sums, lam, estimate) if counts[0] >= s["min_pixels"] else None
            if x is None:
                status = ALIGN_DEGENERATE
                break
            if iters >= s["max_iters"]:
                status = ALIGN_ITERATIONS
                break
            trial, ta, tb = so3.mul(so3.exp(x[:3]), q), a + x[3], b + x[4]
            tsums, tcounts = evaluate(f, trial, ta, tb)
            iters += 1
            take = tcounts[0] >= s["min_pixels"] and tsums[EXPOSURE_COST] / tcounts[0] < sums[EXPOSURE_COST] / counts[0]
            if (estimate & EXPOSURE_GAIN) and not g_lo <= ta <= g_hi:
                take = False
            if take:
                q, a, b, sums, counts = trial, ta, tb, tsums, tcounts
                lam = max(lam / s["lambda_down"], s["lambda_min"])
                if np.linalg.norm(x[:3]) < s["tol_rot"]:
                    status = ALIGN_CONVERGED
                    break
            else:
                lam *= s["lambda_up"]
                if lam > s["lambda_max"]:
                    status = ALIGN_STALLED
                    break
        out["q"][f], out["gain"][f], out["bias"][f], out["sums"][f], out["counts"][f], out["status"][f], out["iters"][f] = q, a, b, sums, counts, status, iters
    return out


def exposure_bytes(frames_u8, gain, bias):
    """exposure_byte (exposure_rule.h) of every byte of frames_u8 [F, S] under its frame's (gain, bias): clamp(rint(a * v + b), 0, 255), ties to even, in
    fp64 — what a compensated frame votes into the mosaic.  uint8 [F, S]."""
    v = np.asarray(frames_u8, dtype=np.uint8)
    F = v.shape[0]
    a, b = exposure_check(gain, bias, F)
    v2 = v.reshape(F, -1).astype(np.float64)
    scaled = a[:, None] * v2
    return np.clip(np.rint(scaled + b[:, None]), 0.0, 255.0).astype(np.uint8)


def exposure_gauge(gain, bias, ok=None):
    """exposure_gauge (exposure_rule.h): the common affine tone of frames aligned to their own mosaic, fixed — alpha = mean a, beta = mean b over the frames
    with ok (all of them where None), a <- a / alpha, b <- (b - beta) / alpha for every frame.  Returns (gain, bias), unchanged copies where no frame is
    ok or alpha is not positive."""
    a, b = np.array(gain, dtype=np.float64).reshape(-1), np.array(bias, dtype=np.float64).reshape(-1)
    sel = np.ones(a.size, bool) if ok is None else np.asarray(ok).astype(bool).reshape(-1)
    if not sel.any():
        return a, b
    alpha, beta = float(np.sum(a[sel])) / int(sel.sum()), float(np.sum(b[sel])) / int(sel.sum())
    if not (alpha > 0.0 and np.isfinite(alpha) and np.isfinite(beta)):
        return a, b
    return a / alpha, (b - beta) / alpha


# ---- intensity frames tracked against their own growing mosaic (numpy forms of emba_frames_track, emba_track_eval and emba_track_level_get,
# include/emba_hip.h; the device forms are LEGM.track_frames, LEGM.track_eval and LEGM.track_level).  The rule is
# emba_amd/csrc/track_rule.h's: given the same level-0 pm the level sums are the same integers; given the same sums and the same level pm the classes are
# the same and the residuals have the same bits.
TRACK_ANCHOR, TRACK_TRACKED, TRACK_LOST = 1, 2, 3      # EMBA_TRACK_*
TRACK_STATUS_NAMES = {1: "anchor", 2: "tracked", 3: "lost"}
TRACK_MAX_LEVEL = 7


def track_level_shape(pano_w, pano_h, level):
    """track_level (track_rule.h): (W_l, H_l, 2^-level) of level 0 ... 7; ValueError where W or H is not divisible by 2^level or fewer than 2 rows are left."""
    W, H, l = int(pano_w), int(pano_h), int(level)
    if not 0 <= l <= TRACK_MAX_LEVEL:
        raise ValueError(f"level = {l}: levels are 0 ... {TRACK_MAX_LEVEL}")
    if W % (1 << l) or H % (1 << l):
        raise ValueError(f"level = {l}: the panorama {W} x {H} is not divisible by {1 << l}")
    if (H >> l) < 2:
        raise ValueError(f"level = {l} leaves {H >> l} rows: a sample needs two")
    return W >> l, H >> l, 1.0 / (1 << l)


def track_level_pm(pm, level):
    """pm_l = pm * 2^-level (exact)."""
    return np.asarray(pm, dtype=np.float64) * (1.0 / (1 << int(level)))


def track_vote_levels(levels):
    """The planes a tracked frame votes into: the schedule's levels in their order, each once, then level 0 where the schedule does not name it."""
    out = []
    for l in levels:
        if int(l) not in out:
            out.append(int(l))
    return out if 0 in out else out + [0]


def track_votes(frames_u8, pm, status, pano_w, pano_h, levels, skip_zero=False):
    """Every level's integer sums from the level-0 pm [F, S, 2] the frames voted with: the frames whose status is TRACK_ANCHOR or TRACK_TRACKED vote through
    mosaic_votes at pm * 2^-l on (W_l, H_l), for every level of track_vote_levels(levels).  A dict of planes {level: (sum_w, sum_v)}, dropped (over every
    plane) and skipped."""
    status = np.asarray(status).reshape(-1)
    F = status.size
    votes = (status == TRACK_ANCHOR) | (status == TRACK_TRACKED)
    fr = np.asarray(frames_u8, dtype=np.uint8).reshape(F, -1)[votes]
    pm = np.asarray(pm, dtype=np.float64).reshape(F, -1, 2)[votes]
    planes, dropped, skipped = {}, 0, 0
    for l in track_vote_levels(levels):
        Wl, Hl, _ = track_level_shape(pano_w, pano_h, l)
        sw, sv, d, skipped = mosaic_votes(fr, track_level_pm(pm, l).reshape(-1, 2), Wl, Hl, skip_zero)
        planes[l] = (sw, sv)
        dropped += d
    return dict(planes=planes, dropped=dropped, skipped=skipped)


def track_terms(frame_u8, pm_l, lut, q, sum_w, sum_v, min_weight=256, skip_zero=False, huber_k=0.0):
    """The terms of one frame's pixels against a level's two sums [H_l, W_l] (track_pixel, track_rule.h) from the level's pm [S, 2]: the plane is
    mosaic_mean of the sums, a pixel is masked when any of its four cells has sum_w < min_weight, the frame's byte is in the plane's units (I = v), and
    J23 is numpy's own on the level's grid.  A dict as align_terms'."""
    mean, covered = mosaic_mean(sum_w, sum_v, min_weight, 0.0)
    return align_terms(frame_u8, pm_l, lut, q, mean, covered, 0.0, 255.0, skip_zero, huber_k)


def track_predict(q_a, t_a, q_b, t_b, t, predict=True):
    """track_predict (track_rule.h): the start of the frame at time t from the last two tracked frames a < b — normalise(exp(omega (t - t_b) / (t_b - t_a))
    (x) q_b), omega = log(q_b (x) q_a^-1); q_b where predict is off or q_a is None."""
    q_b = np.asarray(q_b, dtype=np.float64)
    if not predict or q_a is None:
        return q_b.copy()
    omega = so3.log(so3.mul(q_b, so3.inverse(np.asarray(q_a, dtype=np.float64))))
    u = float(int(t) - int(t_b)) / float(int(t_b) - int(t_a))
    return so3.mul(so3.exp(omega * u), q_b)


def track_frames(frames_u8, frame_t_ns, lut, pano_w, pano_h, q0=(0.0, 0.0, 0.0, 1.0), levels=(0,), batch=1, predict=True, skip_zero=False, min_weight=256,
                 min_overlap=0.5, **settings):
    """The whole tracker of emba_frames_track in numpy, with numpy's own pm: frame 0 is voted at normalise(q0); behind it the frames [f0, f0 + batch) are each
    aligned from their own prediction against the level sums of the frames tracked before f0, level by level through `levels` with align_frames' loop, and
    the tracked ones among them are then voted at every level.  A dict of q [F, 4], status [F], iters [F, len(levels)], cost, overlap [F], counts [F, 4],
    pm [F, S, 2] (the level-0 pm voted with, NaN for a lost frame) and planes {level: (sum_w, sum_v)}.  One difference from the device: batches are cut by
    `batch` alone, not at the device's chunk edges (65 535 frames or 32 MiB of bytes, track_batch_frames of track_rule.h), which calls of this form's size
    do not reach."""
    s = align_settings(**settings)
    W, H = int(pano_w), int(pano_h)
    ts = np.asarray(frame_t_ns, dtype=np.int64).reshape(-1)
    F = ts.size
    if (np.diff(ts) <= 0).any():
        raise ValueError("the frame times must be strictly increasing")
    if int(batch) < 1 or not 0.0 <= float(min_overlap) <= 1.0 or int(min_weight) < 1 or not 1 <= len(levels) <= 8:
        raise ValueError("batch >= 1, 0 <= min_overlap <= 1, min_weight >= 1, 1 ... 8 levels")
    frames = np.asarray(frames_u8, dtype=np.uint8).reshape(F, -1)
    S = frames.shape[1]
    shapes = {l: track_level_shape(W, H, l) for l in track_vote_levels(levels)}
    planes = {l: (np.zeros((Hl, Wl), np.uint64), np.zeros((Hl, Wl), np.uint64)) for l, (Wl, Hl, _) in shapes.items()}
    out = dict(q=np.zeros((F, 4)), status=np.zeros(F, np.int32), iters=np.zeros((F, len(levels)), np.int32), cost=np.zeros(F), overlap=np.zeros(F),
               counts=np.zeros((F, 4), np.int64), pm=np.full((F, S, 2), np.nan), planes=planes)

    def vote(f):
        pm = align_warp(lut, out["q"][f], W, H)[1]
        out["pm"][f] = pm
        for l, (Wl, Hl, scale) in shapes.items():
            sw, sv, _, _ = mosaic_votes(frames[f], pm * scale, Wl, Hl, skip_zero)
            planes[l][0][...] += sw
            planes[l][1][...] += sv

    def evaluate(f, q, l):
        Wl, Hl, scale = shapes[l]
        return align_sums(track_terms(frames[f], align_warp(lut, q, W, H)[1] * scale, lut, q, planes[l][0], planes[l][1], min_weight, skip_zero, s["huber_k"]))

    def align_level(f, q, l):      # align_frames' loop for one frame against one level: (q, sums, counts, status, iters)
        sums, counts = evaluate(f, q, l)
        lam, iters = float(s["lambda0"]), 0
        while True:
            delta = align_step(sums[:6], sums[6:9], lam) if counts[0] >= s["min_pixels"] else None
            if delta is None:
                return q, sums, counts, ALIGN_DEGENERATE, iters
            if iters >= s["max_iters"]:
                return q, sums, counts, ALIGN_ITERATIONS, iters
            trial = so3.mul(so3.exp(delta), q)
            tsums, tcounts = evaluate(f, trial, l)
            iters += 1
            if tcounts[0] >= s["min_pixels"] and tsums[9] / tcounts[0] < sums[9] / counts[0]:
                q, sums, counts = trial, tsums, tcounts
                lam = max(lam / s["lambda_down"], s["lambda_min"])
                if np.linalg.norm(delta) < s["tol_rot"]:
                    return q, sums, counts, ALIGN_CONVERGED, iters
            else:
                lam *= s["lambda_up"]
                if lam > s["lambda_max"]:
                    return q, sums, counts, ALIGN_STALLED, iters

    if not F:
        return out
    out["q"][0], out["status"][0] = so3.normalize(np.asarray(q0, dtype=np.float64)), TRACK_ANCHOR
    vote(0)
    tracked = [0]
    f0 = 1
    while f0 < F:
        nf = min(int(batch), F - f0)
        b = tracked[-1]
        a = tracked[-2] if len(tracked) > 1 else None
        for f in range(f0, f0 + nf):
            pred = track_predict(None if a is None else out["q"][a], None if a is None else ts[a], out["q"][b], ts[b], ts[f], predict)
            q = pred
            for k, l in enumerate(levels):
                q, sums, counts, status, out["iters"][f, k] = align_level(f, q, int(l))
            denom = S - counts[3]
            overlap = counts[0] / denom if denom > 0 else 0.0
            ok = status != ALIGN_DEGENERATE and overlap >= float(min_overlap)
            out["q"][f], out["status"][f] = (q if ok else pred), (TRACK_TRACKED if ok else TRACK_LOST)
            out["cost"][f], out["overlap"][f], out["counts"][f] = sums[9], overlap, counts
        for f in range(f0, f0 + nf):
            if out["status"][f] == TRACK_TRACKED:
                vote(f)
                tracked.append(f)
        f0 += nf
    return out


# ---- the frame tracker with a per-frame exposure (numpy forms of emba_frames_track_exposure and emba_track_exposure_eval, include/emba_hip.h; the device
# forms are LEGM.track_frames_exposure and LEGM.track_exposure_eval).  The rule is emba_amd/csrc/track_exposure_rule.h's, over track_rule.h
# and exposure_rule.h: given the same level-0 pm and the same (gain, bias) the level sums are the same integers; given the same sums and the same level pm the
# classes are the same and the residuals have the same bits.
def track_exposure_terms(frame_u8, pm_l, lut, q, sum_w, sum_v, gain=1.0, bias=0.0, min_weight=256, skip_zero=False, huber_k=0.0):
    """track_terms with the frame's gain and bias (track_exposure_pixel, track_exposure_rule.h): the plane is mosaic_mean of the level's two sums, masked where
    any of a pixel's four cells has sum_w < min_weight, I0 = v (byte units), r = val - (gain * I0 + bias).  exposure_terms' dict, I0 among it."""
    mean, covered = mosaic_mean(sum_w, sum_v, min_weight, 0.0)
    return exposure_terms(frame_u8, pm_l, lut, q, mean, gain, bias, covered, 0.0, 255.0, skip_zero, huber_k)


def track_votes_exposure(frames_u8, pm, status, gain, bias, pano_w, pano_h, levels, skip_zero=False):
    """track_votes of the compensated bytes: the frames whose status is TRACK_ANCHOR or TRACK_TRACKED vote exposure_bytes(v, gain[f], bias[f]) in the place of
    v at pm * 2^-l on (W_l, H_l), for every level of track_vote_levels(levels); skip_zero tests the raw byte.  track_votes' dict."""
    status = np.asarray(status).reshape(-1)
    F = status.size
    votes = (status == TRACK_ANCHOR) | (status == TRACK_TRACKED)
    raw = np.asarray(frames_u8, dtype=np.uint8).reshape(F, -1)[votes]
    a, b = exposure_check(np.asarray(gain, dtype=np.float64).reshape(-1)[votes], np.asarray(bias, dtype=np.float64).reshape(-1)[votes], int(votes.sum()))
    comp = exposure_bytes(raw, a, b).reshape(-1)
    pm = np.asarray(pm, dtype=np.float64).reshape(F, -1, 2)[votes].reshape(-1, 2)
    keep = (raw.reshape(-1) != 0) if skip_zero else np.ones(comp.size, bool)
    planes, dropped = {}, 0
    for l in track_vote_levels(levels):
        Wl, Hl, _ = track_level_shape(pano_w, pano_h, l)
        sw, sv, d, _ = mosaic_votes(comp[keep], track_level_pm(pm[keep], l), Wl, Hl, False)
        planes[l] = (sw, sv)
        dropped += d
    return dict(planes=planes, dropped=dropped, skipped=int((~keep).sum()))


def track_frames_exposure(frames_u8, frame_t_ns, lut, pano_w, pano_h, q0=(0.0, 0.0, 0.0, 1.0), levels=(0,), batch=1, predict=True, skip_zero=False,
                          min_weight=256, min_overlap=0.5, estimate=3, gain_min=None, gain_max=None, **settings):
    """The whole tracker of emba_frames_track_exposure in numpy, with numpy's own pm: track_frames with (a, b) beside every q.  Frame 0 is voted at
    normalise(q0) with a = 1, b = 0; a later frame starts at track_predict's rotation and at the gain and bias of the last tracked frame in front of its
    batch, is aligned level by level with align_frames_exposure's loop (exposure_sums of track_exposure_terms, exposure_step on the rows of `estimate`; every
    level starts where the previous one ended) and, when tracked, votes its compensated bytes at every level.  A lost frame keeps its predicted rotation and
    its start gain and bias.  track_frames' dict, and gain, bias [F]; `levels_degenerate`: the (frame, level) pairs that ended degenerate.  Batches are cut by
    `batch` alone, as in track_frames."""
    s = align_settings(**settings)
    g_lo, g_hi = exposure_bounds(gain_min, gain_max)
    estimate = int(estimate)
    if not 0 <= estimate <= 3:
        raise ValueError("estimate is a mask of EXPOSURE_GAIN and EXPOSURE_BIAS")
    W, H = int(pano_w), int(pano_h)
    ts = np.asarray(frame_t_ns, dtype=np.int64).reshape(-1)
    F = ts.size
    if (np.diff(ts) <= 0).any():
        raise ValueError("the frame times must be strictly increasing")
    if int(batch) < 1 or not 0.0 <= float(min_overlap) <= 1.0 or int(min_weight) < 1 or not 1 <= len(levels) <= 8:
        raise ValueError("batch >= 1, 0 <= min_overlap <= 1, min_weight >= 1, 1 ... 8 levels")
    frames = np.asarray(frames_u8, dtype=np.uint8).reshape(F, -1)
    S = frames.shape[1]
    shapes = {l: track_level_shape(W, H, l) for l in track_vote_levels(levels)}
    planes = {l: (np.zeros((Hl, Wl), np.uint64), np.zeros((Hl, Wl), np.uint64)) for l, (Wl, Hl, _) in shapes.items()}
    out = dict(q=np.zeros((F, 4)), gain=np.ones(F), bias=np.zeros(F), status=np.zeros(F, np.int32), iters=np.zeros((F, len(levels)), np.int32), cost=np.zeros(F),
               overlap=np.zeros(F), counts=np.zeros((F, 4), np.int64), pm=np.full((F, S, 2), np.nan), planes=planes, levels_degenerate=[])

    def vote(f):
        pm = align_warp(lut, out["q"][f], W, H)[1]
        out["pm"][f] = pm
        comp = exposure_bytes(frames[f:f + 1], out["gain"][f:f + 1], out["bias"][f:f + 1]).reshape(-1)
        keep = (frames[f] != 0) if skip_zero else np.ones(S, bool)
        for l, (Wl, Hl, scale) in shapes.items():
            sw, sv, _, _ = mosaic_votes(comp[keep], pm[keep] * scale, Wl, Hl, False)
            planes[l][0][...] += sw
            planes[l][1][...] += sv

    def evaluate(f, q, a, b, l):
        Wl, Hl, scale = shapes[l]
        return exposure_sums(track_exposure_terms(frames[f], align_warp(lut, q, W, H)[1] * scale, lut, q, planes[l][0], planes[l][1], a, b, min_weight, skip_zero,
                                                  s["huber_k"]))

    def align_level(f, q, a, b, l):      # align_frames_exposure's loop for one frame against one level: (q, a, b, sums, counts, status, iters)
        sums, counts = evaluate(f, q, a, b, l)
        lam, iters = float(s["lambda0"]), 0
        while True:
            x = exposure_step(sums, lam, estimate) if counts[0] >= s["min_pixels"] else None
            if x is None:
                return q, a, b, sums, counts, ALIGN_DEGENERATE, iters
            if iters >= s["max_iters"]:
                return q, a, b, sums, counts, ALIGN_ITERATIONS, iters
            trial, ta, tb = so3.mul(so3.exp(x[:3]), q), a + x[3], b + x[4]
            tsums, tcounts = evaluate(f, trial, ta, tb, l)
            iters += 1
            take = tcounts[0] >= s["min_pixels"] and tsums[EXPOSURE_COST] / tcounts[0] < sums[EXPOSURE_COST] / counts[0]
            if (estimate & EXPOSURE_GAIN) and not g_lo <= ta <= g_hi:
                take = False
            if take:
                q, a, b, sums, counts = trial, ta, tb, tsums, tcounts
                lam = max(lam / s["lambda_down"], s["lambda_min"])
                if np.linalg.norm(x[:3]) < s["tol_rot"]:
                    return q, a, b, sums, counts, ALIGN_CONVERGED, iters
            else:
                lam *= s["lambda_up"]
                if lam > s["lambda_max"]:
                    return q, a, b, sums, counts, ALIGN_STALLED, iters

    if not F:
        return out
    out["q"][0], out["status"][0] = so3.normalize(np.asarray(q0, dtype=np.float64)), TRACK_ANCHOR
    vote(0)
    tracked = [0]
    f0 = 1
    while f0 < F:
        nf = min(int(batch), F - f0)
        tb_ = tracked[-1]
        ta_ = tracked[-2] if len(tracked) > 1 else None
        a0, b0 = float(out["gain"][tb_]), float(out["bias"][tb_])
        for f in range(f0, f0 + nf):
            pred = track_predict(None if ta_ is None else out["q"][ta_], None if ta_ is None else ts[ta_], out["q"][tb_], ts[tb_], ts[f], predict)
            q, a, b = pred, a0, b0
            for k, l in enumerate(levels):
                q, a, b, sums, counts, status, out["iters"][f, k] = align_level(f, q, a, b, int(l))
                if status == ALIGN_DEGENERATE:
                    out["levels_degenerate"].append((f, int(l)))
            denom = S - counts[3]
            overlap = counts[0] / denom if denom > 0 else 0.0
            ok = status != ALIGN_DEGENERATE and overlap >= float(min_overlap)
            out["q"][f], out["status"][f] = (q if ok else pred), (TRACK_TRACKED if ok else TRACK_LOST)
            out["gain"][f], out["bias"][f] = (a, b) if ok else (a0, b0)
            out["cost"][f], out["overlap"][f], out["counts"][f] = sums[EXPOSURE_COST], overlap, counts
        for f in range(f0, f0 + nf):
            if out["status"][f] == TRACK_TRACKED:
                vote(f)
                tracked.append(f)
        f0 += nf
    return out


# ---- tracked frames refitted against the mosaic of the other frames (the numpy form of emba_frames_refit, include/emba_hip.h; the device form is
# LEGM.refit_frames).  The rule is emba_amd/csrc/refit_rule.h's, over the trackers': the level sums are unsigned 64-bit integers, a frame's
# votes leave them by subtraction modulo 2^64, and given the device's pm and (gain, bias) track_votes_exposure gives the device's integers.
REFIT_ANCHOR, REFIT_MOVED, REFIT_KEPT, REFIT_RECOVERED, REFIT_LOST = 1, 2, 3, 4, 5      # EMBA_REFIT_*
REFIT_NAMES = {0: "-", 1: "anchor", 2: "moved", 3: "kept", 4: "recovered", 5: "lost"}


def refit_batches(F, batch):
    """The batches of F frames as the trackers cut them (track_batch_frames without the chunk edges): frame 0 alone, then `batch` frames each: [(f0, nf)]."""
    out, f0 = [], 0
    while f0 < F:
        nf = 1 if f0 == 0 else min(int(batch), F - f0)
        out.append((f0, nf))
        f0 += nf
    return out


def refit_start(status, ts, q, gain, bias, f):
    """refit_start (refit_rule.h): where frame f starts — a voting frame at its own (q, a, b); a lost frame from the nearest voting frames a < f < b by
    index: track_predict's formula at t_f (its factor is negative: an interpolation) with gain and bias linear in the same factor, or the values of the
    one neighbour there is.  (q, a, b), or None where no frame votes."""
    status = np.asarray(status).reshape(-1)
    votes = (status == TRACK_ANCHOR) | (status == TRACK_TRACKED)
    if votes[f]:
        return np.array(q[f], dtype=np.float64), float(gain[f]), float(bias[f])
    before, after = np.flatnonzero(votes[:f]), f + 1 + np.flatnonzero(votes[f + 1:])
    if not before.size and not after.size:
        return None
    if not before.size or not after.size:
        o = int(after[0] if not before.size else before[-1])
        return np.array(q[o], dtype=np.float64), float(gain[o]), float(bias[o])
    a, b = int(before[-1]), int(after[0])
    u = float(int(ts[f]) - int(ts[b])) / float(int(ts[b]) - int(ts[a]))
    return track_predict(q[a], ts[a], q[b], ts[b], ts[f], True), float(gain[b] + (gain[b] - gain[a]) * u), float(bias[b] + (bias[b] - bias[a]) * u)


def _exposure_align_level(evaluate, q, a, b, s, estimate, g_lo, g_hi):
    """align_frames_exposure's loop for one frame against one level (track_frames_exposure runs the same): (q, a, b, sums, counts, status, iters)."""
    sums, counts = evaluate(q, a, b)
    lam, iters = float(s["lambda0"]), 0
    while True:
        x = exposure_step(sums, lam, estimate) if counts[0] >= s["min_pixels"] else None
        if x is None:
            return q, a, b, sums, counts, ALIGN_DEGENERATE, iters
        if iters >= s["max_iters"]:
            return q, a, b, sums, counts, ALIGN_ITERATIONS, iters
        trial, ta, tb = so3.mul(so3.exp(x[:3]), q), a + x[3], b + x[4]
        tsums, tcounts = evaluate(trial, ta, tb)
        iters += 1
        take = tcounts[0] >= s["min_pixels"] and tsums[EXPOSURE_COST] / tcounts[0] < sums[EXPOSURE_COST] / counts[0]
        if (estimate & EXPOSURE_GAIN) and not g_lo <= ta <= g_hi:
            take = False
        if take:
            q, a, b, sums, counts = trial, ta, tb, tsums, tcounts
            lam = max(lam / s["lambda_down"], s["lambda_min"])
            if np.linalg.norm(x[:3]) < s["tol_rot"]:
                return q, a, b, sums, counts, ALIGN_CONVERGED, iters
        else:
            lam *= s["lambda_up"]
            if lam > s["lambda_max"]:
                return q, a, b, sums, counts, ALIGN_STALLED, iters


def refit_frames(frames_u8, frame_t_ns, lut, pano_w, pano_h, q, status, gain=None, bias=None, levels=(0,), batch=1, sweeps=1, alternate=True, recover=True,
                 sweep_tol=0.0, estimate=0, skip_zero=False, min_weight=256, min_overlap=0.5, gain_min=None, gain_max=None, **settings):
    """The whole refit of emba_frames_refit in numpy, with numpy's own pm.  The planes are built from every voting frame at its given (q, a, b)
    (track_votes_exposure).  A sweep visits the batches (refit_batches; with `alternate` the odd sweeps backwards): the tracked frames of the batch take
    their votes out of the uint64 sums again (subtraction modulo 2^64), every active frame — tracked, or lost under `recover` — starts at refit_start and
    is aligned level by level by track_frames_exposure's loop against what is left, and the verdict moves it, keeps it, recovers it or leaves it lost; the
    tracked frames of the batch are then voted back.  A dict of q, gain, bias, status, refit [F] (REFIT_*), iters [F, len(levels)], cost, overlap, counts
    (the last sweep's), sweep [sweeps_done, 4] (moved, recovered, largest rotation change, sum of the last-level costs), sweeps_done, iters_sweeps
    [sweeps_done, len(levels)] (trials per level summed over the frames), refit_sweeps [sweeps_done, F], pm [F, S, 2], planes {level: (sum_w, sum_v)},
    dropped and skipped.  Batches are cut by `batch` alone, as in track_frames."""
    s = align_settings(**settings)
    g_lo, g_hi = exposure_bounds(gain_min, gain_max)
    estimate, sweeps = int(estimate), int(sweeps)
    if not 0 <= estimate <= 3:
        raise ValueError("estimate is a mask of EXPOSURE_GAIN and EXPOSURE_BIAS")
    W, H = int(pano_w), int(pano_h)
    ts = np.asarray(frame_t_ns, dtype=np.int64).reshape(-1)
    F = ts.size
    if (np.diff(ts) <= 0).any():
        raise ValueError("the frame times must be strictly increasing")
    if int(batch) < 1 or not 0.0 <= float(min_overlap) <= 1.0 or int(min_weight) < 1 or not 1 <= len(levels) <= 8:
        raise ValueError("batch >= 1, 0 <= min_overlap <= 1, min_weight >= 1, 1 ... 8 levels")
    if sweeps < 0 or not float(sweep_tol) >= 0.0:
        raise ValueError("sweeps >= 0, sweep_tol >= 0")
    frames = np.asarray(frames_u8, dtype=np.uint8).reshape(F, -1)
    S = frames.shape[1]
    q = np.array(q, dtype=np.float64).reshape(F, 4)
    status = np.array(status, dtype=np.int32).reshape(F)
    gain = np.broadcast_to(np.asarray(1.0 if gain is None else gain, dtype=np.float64), (F,)).copy()
    bias = np.broadcast_to(np.asarray(0.0 if bias is None else bias, dtype=np.float64), (F,)).copy()
    # refit_args_ok's refusals, in its order
    if not np.isin(status, (TRACK_ANCHOR, TRACK_TRACKED, TRACK_LOST)).all():
        raise ValueError("a status is TRACK_ANCHOR, TRACK_TRACKED or TRACK_LOST")
    if not np.isin(status, (TRACK_ANCHOR, TRACK_TRACKED)).any():
        raise ValueError("no frame votes: a refit needs an anchor or a tracked frame")
    for f in range(F):
        n2 = float((q[f] * q[f]).sum())
        if not (np.isfinite(n2) and n2 > 0.0):
            raise ValueError(f"q[{f}] is not finite or has zero norm")
        if not (np.isfinite(gain[f]) and g_lo <= gain[f] <= g_hi):
            raise ValueError(f"gain[{f}] = {gain[f]} is not finite or outside the bounds")
        if not np.isfinite(bias[f]):
            raise ValueError(f"bias[{f}] is not finite")
    vote_levels = track_vote_levels(levels)
    shapes = {l: track_level_shape(W, H, l) for l in vote_levels}
    planes = {l: (np.zeros((Hl, Wl), np.uint64), np.zeros((Hl, Wl), np.uint64)) for l, (Wl, Hl, _) in shapes.items()}
    pm = np.full((F, S, 2), np.nan)
    counters = [0, 0]
    mask = (1 << 64) - 1

    def vote(f, negate=False):
        if not negate:
            pm[f] = align_warp(lut, q[f], W, H)[1]
        v = track_votes_exposure(frames[f:f + 1], pm[f:f + 1], [TRACK_TRACKED], gain[f:f + 1], bias[f:f + 1], W, H, levels, skip_zero)
        for l in vote_levels:
            for k in (0, 1):
                if negate:
                    planes[l][k][...] -= v["planes"][l][k]      # (uint64: modulo 2^64)
                else:
                    planes[l][k][...] += v["planes"][l][k]
        for k, name in enumerate(("dropped", "skipped")):
            counters[k] = (counters[k] + (-v[name] if negate else v[name])) & mask

    def evaluate_at(f, l):
        _, _, scale = shapes[l]
        return lambda qq, aa, bb: exposure_sums(track_exposure_terms(frames[f], align_warp(lut, qq, W, H)[1] * scale, lut, qq, planes[l][0], planes[l][1], aa, bb,
                                                                     min_weight, skip_zero, s["huber_k"]))

    votes_now = lambda: (status == TRACK_ANCHOR) | (status == TRACK_TRACKED)      # noqa: E731
    for f in np.flatnonzero(votes_now()):
        vote(int(f))
    refit = np.where(status == TRACK_ANCHOR, REFIT_ANCHOR, np.where(status == TRACK_LOST, REFIT_LOST, 0)).astype(np.int32)
    iters, cost, overlap, counts = np.zeros((F, len(levels)), np.int32), np.zeros(F), np.zeros(F), np.zeros((F, 4), np.int64)
    sweep_rows, iters_sweeps, refit_sweeps = [], [], []
    batches = refit_batches(F, batch)
    for sweep in range(sweeps):
        q_before = q.copy()
        refit = np.where(status == TRACK_ANCHOR, REFIT_ANCHOR, np.where(status == TRACK_LOST, REFIT_LOST, 0)).astype(np.int32)
        iters[...], cost[...], overlap[...], counts[...] = 0, 0.0, 0.0, 0
        for f0, nf in (batches[::-1] if alternate and sweep & 1 else batches):
            fs = range(f0, f0 + nf)
            entered = status.copy()
            active = [f for f in fs if entered[f] == TRACK_TRACKED or (recover and entered[f] == TRACK_LOST)]
            for f in fs:
                if entered[f] == TRACK_TRACKED:
                    vote(f, negate=True)
            starts = {f: refit_start(entered, ts, q, gain, bias, f) for f in active}
            new = {}
            for f in active:
                qq, aa, bb = starts[f]
                for k, l in enumerate(levels):
                    qq, aa, bb, sums, cnt, st, iters[f, k] = _exposure_align_level(evaluate_at(f, int(l)), qq, aa, bb, s, estimate, g_lo, g_hi)
                denom = S - cnt[3]
                overlap[f] = cnt[0] / denom if denom > 0 else 0.0
                cost[f], counts[f] = sums[EXPOSURE_COST], cnt
                passed = st != ALIGN_DEGENERATE and overlap[f] >= float(min_overlap)
                was_lost = entered[f] == TRACK_LOST
                refit[f] = (REFIT_RECOVERED if was_lost else REFIT_MOVED) if passed else (REFIT_LOST if was_lost else REFIT_KEPT)
                if passed:
                    new[f] = (qq, aa, bb)
            for f, (qq, aa, bb) in new.items():
                q[f], gain[f], bias[f], status[f] = qq, aa, bb, TRACK_TRACKED
            for f in fs:
                if status[f] == TRACK_TRACKED:
                    vote(f)
        change = float(rotation_angle_between(q_before, q).max())
        sweep_rows.append([float((refit == REFIT_MOVED).sum()), float((refit == REFIT_RECOVERED).sum()), change, float(cost.sum())])
        iters_sweeps.append(iters.sum(axis=0))
        refit_sweeps.append(refit.copy())
        if change < float(sweep_tol):
            break
    pm[~votes_now()] = np.nan
    n_lv = len(levels)
    return dict(q=q, gain=gain, bias=bias, status=status, refit=refit, iters=iters, cost=cost, overlap=overlap, counts=counts,
                sweep=np.array(sweep_rows, dtype=np.float64).reshape(-1, 4), sweeps_done=len(sweep_rows),
                iters_sweeps=np.array(iters_sweeps, dtype=np.int64).reshape(-1, n_lv), refit_sweeps=np.array(refit_sweeps, dtype=np.int32).reshape(-1, F), pm=pm,
                planes=planes, dropped=counters[0], skipped=counters[1])


def rotation_angle_between(qa, qb):
    """The angle (rad) of the rotation from qa to qb, quaternions xyzw [..., 4]."""
    qa, qb = np.asarray(qa, dtype=np.float64).reshape(-1, 4), np.asarray(qb, dtype=np.float64).reshape(-1, 4)
    return np.array([np.linalg.norm(so3.log(so3.mul(b, so3.inverse(a)))) for a, b in zip(qa, qb)])


# ---- loops closed among tracked frames (numpy forms of emba_frames_pair_eval, emba_frames_pair_align and emba_rotation_graph_solve, include/emba_hip.h; the
# device forms are LEGM.pair_eval and LEGM.pair_align, the host form LEGM.rotation_graph_solve).  The rules are emba_amd/csrc/pair_rule.h's
# and graph_rule.h's: given the same uv, the classes are the same and the residuals have the same bits.  rb, uv and the Jacobians are numpy's own.
PAIR_MAX_BYTES = 1 << 30                 # kPairMaxBytes: the resident sequence of a call
PAIR_MAX_CANDIDATE_FRAMES = 4096         # pair_candidates is O(F^2) on the host: 16 M angles at the bound
GRAPH_CONVERGED, GRAPH_STALLED, GRAPH_ITERATIONS, GRAPH_DEGENERATE = 1, 2, 3, 4      # EMBA_GRAPH_*
GRAPH_END_NAMES = {1: "converged", 2: "stalled", 3: "iterations", 4: "degenerate"}
GRAPH_DEFAULTS = dict(max_iters=50, cg_max_iters=200, lambda0=1e-4, lambda_up=10.0, lambda_down=10.0, lambda_min=1e-12, lambda_max=1e8, tol=1e-10, cg_tol=1e-10)
TRACK_ANCHOR = 1                         # EMBA_TRACK_ANCHOR
PAIR_NOISE_FLOOR = 1.0 / 12.0            # the variance of a byte's rounding: the floor close_tracked_frames puts under a pair's s^2


def pair_calib(fu, fv, cu, cv, D=None):
    """The camera of a pair call: a dict of fu, fv, cu, cv and D (k1, k2, p1, p2, k3 as bearing_lut_from_calibration takes them; None: the pinhole)."""
    return dict(fu=float(fu), fv=float(fv), cu=float(cu), cv=float(cv), D=None if D is None else np.concatenate([np.asarray(D, np.float64).ravel(), np.zeros(5)])[:5])


def pair_start(q, gain, bias, pairs):
    """(Q [P, 4], a [P], b [P]) of the pairs (i, j) from per-frame camera-to-world rotations q [F, 4] and exposures: Q = q_j^-1 (x) q_i, a = a_i / a_j,
    b = (b_i - b_j) / a_j (gain, bias: [F], or None for 1 and 0)."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 4)
    F = q.shape[0]
    g = np.ones(F) if gain is None else np.broadcast_to(np.asarray(gain, dtype=np.float64), (F,))
    o = np.zeros(F) if bias is None else np.broadcast_to(np.asarray(bias, dtype=np.float64), (F,))
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    Q = np.array([so3.mul(so3.inverse(q[j]), q[i]) for i, j in pairs]).reshape(-1, 4)
    i, j = pairs[:, 0], pairs[:, 1]
    return Q, g[i] / g[j], (o[i] - o[j]) / g[j]


def pair_project(lut, Q, calib):
    """numpy's own projection of one pair: rb = R(Q) lut [S, 3]; uv [S, 2] through the plumb_bob model (NaN where rb_z <= 0); J23 [S, 2, 3] = d(u, v) / d rb;
    Ju [S, 2, 3] = J23 (-[rb]x), the Jacobian for Q <- exp(delta) Q."""
    from . import synth
    lut = np.asarray(lut, dtype=np.float64).reshape(-1, 3)
    rb = lut @ synth._quat_to_R(so3.normalize(Q)).T
    z = rb[:, 2]
    ok = z > 0.0
    zs = np.where(ok, z, 1.0)
    x, y = rb[:, 0] / zs, rb[:, 1] / zs
    D = calib.get("D")
    k1, k2, p1, p2, k3 = np.zeros(5) if D is None else D
    fu, fv, cu, cv = calib["fu"], calib["fv"], calib["cu"], calib["cv"]
    r2 = x * x + y * y
    radial = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * radial + (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))
    yd = y * radial + (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)
    uv = np.stack([np.where(ok, fu * xd + cu, np.nan), np.where(ok, fv * yd + cv, np.nan)], axis=1)
    rd = (3.0 * k3 * r2 + 2.0 * k2) * r2 + k1
    cross = 2.0 * x * y * rd + 2.0 * p1 * x + 2.0 * p2 * y
    axx = radial + 2.0 * x * x * rd + 2.0 * p1 * y + 6.0 * p2 * x
    ayy = radial + 2.0 * y * y * rd + 6.0 * p1 * y + 2.0 * p2 * x
    iz = 1.0 / zs
    J23 = np.stack([np.stack([fu * axx * iz, fu * cross * iz, -fu * (axx * x + cross * y) * iz], axis=1),
                    np.stack([fv * cross * iz, fv * ayy * iz, -fv * (cross * x + ayy * y) * iz], axis=1)], axis=1)
    zero = np.zeros_like(z)
    M = np.stack([np.stack([zero, rb[:, 2], -rb[:, 1]], axis=1), np.stack([-rb[:, 2], zero, rb[:, 0]], axis=1), np.stack([rb[:, 1], -rb[:, 0], zero], axis=1)], axis=1)
    return rb, uv, J23, J23 @ M


def pair_terms(src_u8, tgt_u8, uv, lut, Q, calib, gain=1.0, bias=0.0, skip_zero=False, huber_k=0.0):
    """The terms of one pair's source pixels (pair_pixel, pair_rule.h) from a given uv [S, 2] (the device's uv_out, or pair_project's) and numpy's own Ju of
    Q: src_u8 [S] the source frame, tgt_u8 [sh, sw] the target frame.  A dict as align_terms': cls (ALIGN_USED / OUTSIDE / MASKED / SKIPPED, in this
    precedence; masked and skipped only with skip_zero), r = val - (gain v + bias), w, rho, g [S, 3]."""
    T = np.asarray(tgt_u8, dtype=np.uint8)
    sh, sw = T.shape
    v = np.asarray(src_u8, dtype=np.uint8).reshape(-1)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    if uv.shape[0] != v.size:
        raise ValueError(f"uv has {uv.shape[0]} rows, the frame has {v.size} pixels")
    with np.errstate(invalid="ignore"):
        fin = (np.abs(uv[:, 0]) < 2147483648.0) & (np.abs(uv[:, 1]) < 2147483648.0)
    x, y = np.where(fin, uv[:, 0], -1.0), np.where(fin, uv[:, 1], -1.0)
    fx, fy = np.floor(x), np.floor(y)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    inside = fin & (ix >= 0) & (ix + 1 <= sw - 1) & (iy >= 0) & (iy + 1 <= sh - 1)
    ix, iy = np.where(inside, ix, 0), np.where(inside, iy, 0)
    ax, ay = x - fx, y - fy
    b00, b01, b10, b11 = T[iy, ix], T[iy, ix + 1], T[iy + 1, ix], T[iy + 1, ix + 1]
    p00, p01, p10, p11 = (b.astype(np.float64) for b in (b00, b01, b10, b11))
    top = (1.0 - ax) * p00 + ax * p01
    bot = (1.0 - ax) * p10 + ax * p11
    val = (1.0 - ay) * top + ay * bot
    gx = (1.0 - ay) * (p01 - p00) + ay * (p11 - p10)
    gy = (1.0 - ax) * (p10 - p00) + ax * (p11 - p01)
    cls = np.full(v.size, ALIGN_USED, dtype=np.int64)
    if skip_zero:
        cls[v == 0] = ALIGN_SKIPPED
        cls[(b00 == 0) | (b01 == 0) | (b10 == 0) | (b11 == 0)] = ALIGN_MASKED
    cls[~inside] = ALIGN_OUTSIDE
    used = cls == ALIGN_USED
    r = np.where(used, val - (float(gain) * v.astype(np.float64) + float(bias)), 0.0)
    w, rho = align_huber(r, huber_k)
    Ju = pair_project(lut, Q, calib)[3]
    g = gx[:, None] * Ju[:, 0, :] + gy[:, None] * Ju[:, 1, :]
    return dict(cls=cls, r=r, w=np.where(used, w, 0.0), rho=np.where(used, rho, 0.0), g=np.where(used[:, None], g, 0.0))


def pair_sums(terms, with_scale=False):
    """The ten sums and the four counts of one pair's terms: align_sums."""
    return align_sums(terms, with_scale)


def pair_information(sums, counts, floor=0.0):
    """Lambda [..., 6] = H / s^2 (00 01 02 11 12 22) with s^2 = cost / max(n - 3, 1), of sums [..., 10] and counts [..., 4] (or n itself).  floor: a lower
    bound on s^2 (byte units squared), 0 for the rule as it stands; PAIR_NOISE_FLOOR is the variance a byte's rounding alone leaves, what two frames that
    happen to agree bit for bit (s^2 = 0, an infinite information) still differ by."""
    sums = np.asarray(sums, dtype=np.float64)
    n = np.asarray(counts, dtype=np.int64)
    n = n[..., 0] if n.ndim == sums.ndim else n
    with np.errstate(divide="ignore", invalid="ignore"):
        s2 = np.maximum(sums[..., 9] / np.maximum(n - 3, 1).astype(np.float64), float(floor))
        return sums[..., :6] / s2[..., None]


def pair_align(frames_u8, pairs, Q_xyzw, lut, calib, sensor, gain=None, bias=None, skip_zero=False, **settings):
    """The loop of emba_frames_pair_align in numpy, with numpy's own uv: per pair (i, j) of frames_u8 [F, S] the Levenberg-Marquardt iteration of align_step
    (align_rule.h) on pair_terms' sums, as align_frames runs it.  sensor: (sw, sh).  A dict of q [P, 4], sums [P, 10], counts [P, 4], status, iters, cost0,
    n0 [P] and info [P, 6]."""
    s = align_settings(**settings)
    sw, sh = int(sensor[0]), int(sensor[1])
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    P = pairs.shape[0]
    Q_in = np.asarray(Q_xyzw, dtype=np.float64).reshape(P, 4)
    frames = np.asarray(frames_u8, dtype=np.uint8).reshape(-1, sh * sw)
    a = np.ones(P) if gain is None else np.broadcast_to(np.asarray(gain, dtype=np.float64), (P,))
    b = np.zeros(P) if bias is None else np.broadcast_to(np.asarray(bias, dtype=np.float64), (P,))

    def evaluate(p, q):
        i, j = pairs[p]
        return pair_sums(pair_terms(frames[i], frames[j].reshape(sh, sw), pair_project(lut, q, calib)[1], lut, q, calib, a[p], b[p], skip_zero, s["huber_k"]))

    out = dict(q=Q_in.copy(), sums=np.zeros((P, 10)), counts=np.zeros((P, 4), np.int64), status=np.zeros(P, np.int32), iters=np.zeros(P, np.int32),
               cost0=np.zeros(P), n0=np.zeros(P, np.int64))
    for p in range(P):
        q = Q_in[p].copy()
        sums, counts = evaluate(p, q)
        out["cost0"][p], out["n0"][p] = sums[9], counts[0]
        lam, iters = float(s["lambda0"]), 0
        while True:
            delta = align_step(sums[:6], sums[6:9], lam) if counts[0] >= s["min_pixels"] else None
            if delta is None:
                status = ALIGN_DEGENERATE
                break
            if iters >= s["max_iters"]:
                status = ALIGN_ITERATIONS
                break
            trial = so3.mul(so3.exp(delta), q)
            tsums, tcounts = evaluate(p, trial)
            iters += 1
            if tcounts[0] >= s["min_pixels"] and tsums[9] / tcounts[0] < sums[9] / counts[0]:
                q, sums, counts = trial, tsums, tcounts
                lam = max(lam / s["lambda_down"], s["lambda_min"])
                if np.linalg.norm(delta) < s["tol_rot"]:
                    status = ALIGN_CONVERGED
                    break
            else:
                lam *= s["lambda_up"]
                if lam > s["lambda_max"]:
                    status = ALIGN_STALLED
                    break
        out["q"][p], out["sums"][p], out["counts"][p], out["status"][p], out["iters"][p] = q, sums, counts, status, iters
    out["info"] = pair_information(out["sums"], out["counts"])
    return out


# ---- the pair alignment coarse to fine over a pyramid of the sensor frames, with the pair's exposure estimated (numpy forms of emba_frames_pair_level_eval
# and emba_frames_pair_align_levels, include/emba_hip.h; the device forms are LEGM.pair_level_eval and LEGM.pair_align_levels).  The rules are
# emba_amd/csrc/pair_level_rule.h's: the level bytes are equal integers, the level table and the level camera have the same bits.
PAIR_MAX_LEVEL = 7                       # kPairMaxLevel
PAIR_MAX_LEVELS = 8                      # kPairMaxLevels: entries of a schedule
PAIR_EXPOSURE_MODES = {"none": 0, "bias": EXPOSURE_BIAS, "gain-bias": EXPOSURE_GAIN | EXPOSURE_BIAS}


def pair_level_size(sensor, level):
    """(sw >> l, sh >> l) of sensor = (sw, sh); ValueError for a level outside 0 ... PAIR_MAX_LEVEL or one below 2 x 2 (a bilinear cell needs 2 x 2)."""
    sw, sh, l = int(sensor[0]), int(sensor[1]), int(level)
    if not 0 <= l <= PAIR_MAX_LEVEL:
        raise ValueError(f"level {l} is outside 0 ... {PAIR_MAX_LEVEL}")
    if (sw >> l) < 2 or (sh >> l) < 2:
        raise ValueError(f"level {l} of a {sw} x {sh} sensor is {sw >> l} x {sh >> l}: a bilinear cell needs 2 x 2")
    return sw >> l, sh >> l


def pair_check_levels(levels, sensor):
    """The schedule as a tuple of ints; the refusals of emba_frames_pair_align_levels' schedule as ValueError."""
    lv = tuple(int(l) for l in np.asarray(levels).reshape(-1))
    if not 1 <= len(lv) <= PAIR_MAX_LEVELS:
        raise ValueError(f"a schedule has 1 ... {PAIR_MAX_LEVELS} levels, not {len(lv)}")
    for l in lv:
        if not 0 <= l <= PAIR_MAX_LEVEL:
            raise ValueError(f"level {l} is outside 0 ... {PAIR_MAX_LEVEL}")
    for l in lv:
        pair_level_size(sensor, l)
    return lv


def pair_level_bytes(frames_u8, level, skip_zero=False):
    """Level `level` of frames_u8 [..., sh, sw]: uint8 [..., sh >> l, sw >> l], (sum of the box + 4^l / 2) >> 2l in integers from level 0 directly; under
    skip_zero a box that holds a zero byte is 0.  The columns and rows left over at the right and at the bottom take no part."""
    fr = np.asarray(frames_u8, dtype=np.uint8)
    sh, sw = fr.shape[-2:]
    wl, hl = pair_level_size((sw, sh), level)
    l = int(level)
    if l == 0:
        return fr.copy()
    n = 1 << l
    box = fr[..., :hl * n, :wl * n].reshape(fr.shape[:-2] + (hl, n, wl, n))
    out = (box.astype(np.int64).sum(axis=(-3, -1)) + ((1 << (2 * l)) >> 1)) >> (2 * l)
    if skip_zero:
        out = np.where((box == 0).any(axis=(-3, -1)), 0, out)
    return out.astype(np.uint8)


def pair_level_lut(lut, sensor, level):
    """The bearing table [S_l, 3] of level `level` from the table lut [S, 3] of sensor = (sw, sh): level 0 the table; above it 0.25 ((b00 + b01) + (b10 +
    b11)) of the four pixels around the centre of each box, componentwise in this order."""
    sw, sh = int(sensor[0]), int(sensor[1])
    wl, hl = pair_level_size(sensor, level)
    l = int(level)
    T = np.asarray(lut, dtype=np.float64).reshape(sh, sw, 3)
    if l == 0:
        return T.reshape(-1, 3).copy()
    h = 1 << (l - 1)
    ys, xs = np.arange(hl) * 2 * h + h - 1, np.arange(wl) * 2 * h + h - 1
    b00, b01 = T[ys[:, None], xs[None, :]], T[ys[:, None], xs[None, :] + 1]
    b10, b11 = T[ys[:, None] + 1, xs[None, :]], T[ys[:, None] + 1, xs[None, :] + 1]
    return (0.25 * ((b00 + b01) + (b10 + b11))).reshape(-1, 3)


def pair_level_calib(calib, level):
    """The camera of level `level`: fu / 2^l, fv / 2^l, (cu - (2^l - 1) / 2) / 2^l, cv likewise, D unchanged.  Level 0 is the camera bit for bit."""
    l = int(level)
    if not 0 <= l <= PAIR_MAX_LEVEL:
        raise ValueError(f"level {l} is outside 0 ... {PAIR_MAX_LEVEL}")
    n, half = float(1 << l), (float(1 << l) - 1.0) / 2.0
    return dict(fu=float(calib["fu"]) / n, fv=float(calib["fv"]) / n, cu=(float(calib["cu"]) - half) / n, cv=(float(calib["cv"]) - half) / n, D=calib.get("D"))


def pair_level_min_pixels(min_pixels, level):
    """min_pixels at a level: min_pixels >> 2l, but not below the smaller of min_pixels and 8."""
    return max(int(min_pixels) >> (2 * int(level)), min(int(min_pixels), 8))


def pair_exposure_terms(src_u8, tgt_u8, uv, lut, Q, calib, gain=1.0, bias=0.0, skip_zero=False, huber_k=0.0):
    """pair_terms with the exposure's column: its dict and I0 [S] = the source byte as a double (0 where the pixel is not used).  The Jacobian row of r in
    (delta, a, b) is (g, -I0, -1).  Everything is the level's: bytes, uv, table and camera."""
    t = pair_terms(src_u8, tgt_u8, uv, lut, Q, calib, gain, bias, skip_zero, huber_k)
    v = np.asarray(src_u8, dtype=np.uint8).reshape(-1).astype(np.float64)
    t["I0"] = np.where(t["cls"] == ALIGN_USED, v, 0.0)
    return t


def pair_exposure_sums(terms, with_scale=False):
    """The 21 sums and the four counts of one pair's terms: exposure_sums."""
    return exposure_sums(terms, with_scale)


def pair_align_levels(frames_u8, pairs, Q_xyzw, lut, calib, sensor, levels=(0,), estimate=0, gain=None, bias=None, skip_zero=False, gain_min=None, gain_max=None,
                      order=None, **settings):
    """The schedule of emba_frames_pair_align_levels in numpy, with numpy's own uv: per pair (i, j) of frames_u8 [F, S], level by level through `levels`, the
    loop of align_frames_exposure (exposure_step on pair_exposure_sums) on the level's bytes, table and camera, min_pixels by pair_level_min_pixels; level
    k + 1 starts from the accepted (Q, a, b) of level k; a level that ends degenerate ends the pair.  sensor: (sw, sh).  order: a function n -> a permutation
    of a level's n pixels, in which the sums are then taken in plain fp64 (None: np.longdouble in pixel order) — what measures the spread of the result under
    the order of summation.  A dict of q [P, 4], gain, bias [P], sums [P, 21], counts [P, 4], status, iters [P], level_status, level_iters [P, n], cost0, n0
    [P], info [P, 6] and last_x [P, 5]: the last accepted step (delta, x_a, x_b) of the last level run, what the stopping rule leaves undetermined."""
    s = align_settings(**settings)
    g_lo, g_hi = exposure_bounds(gain_min, gain_max)
    estimate = int(estimate)
    if not 0 <= estimate <= 3:
        raise ValueError("estimate is a mask of EXPOSURE_GAIN and EXPOSURE_BIAS")
    sw, sh = int(sensor[0]), int(sensor[1])
    lv = pair_check_levels(levels, sensor)
    n = len(lv)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    P = pairs.shape[0]
    Q_in = np.asarray(Q_xyzw, dtype=np.float64).reshape(P, 4)
    frames = np.asarray(frames_u8, dtype=np.uint8).reshape(-1, sh, sw)
    a_in = np.ones(P) if gain is None else np.broadcast_to(np.asarray(gain, dtype=np.float64), (P,))
    b_in = np.zeros(P) if bias is None else np.broadcast_to(np.asarray(bias, dtype=np.float64), (P,))
    pyramid = {l: (pair_level_bytes(frames, l, skip_zero), pair_level_lut(lut, sensor, l), pair_level_calib(calib, l)) for l in set(lv)}

    def evaluate(l, p, q, a, b):
        fb, tl, cl = pyramid[l]
        i, j = pairs[p]
        t = pair_exposure_terms(fb[i].reshape(-1), fb[j], pair_project(tl, q, cl)[1], tl, q, cl, a, b, skip_zero, s["huber_k"])
        if order is None:
            return pair_exposure_sums(t)
        perm = np.asarray(order(t["cls"].size))      # (... and plain fp64 one term after the other, where pair_exposure_sums accumulates in np.longdouble)
        return np.cumsum(exposure_sum_terms(t)[perm], axis=0)[-1], np.bincount(t["cls"], minlength=4).astype(np.int64)

    out = dict(q=Q_in.copy(), gain=a_in.copy(), bias=b_in.copy(), sums=np.zeros((P, EXPOSURE_SUMS)), counts=np.zeros((P, 4), np.int64), status=np.zeros(P, np.int32),
               iters=np.zeros(P, np.int32), level_status=np.zeros((P, n), np.int32), level_iters=np.zeros((P, n), np.int32), cost0=np.zeros(P), n0=np.zeros(P, np.int64),
               last_x=np.zeros((P, 5)))
    for p in range(P):
        q, a, b = Q_in[p].copy(), float(a_in[p]), float(b_in[p])
        for k, l in enumerate(lv):
            out["last_x"][p] = 0.0
            min_pixels = pair_level_min_pixels(s["min_pixels"], l)
            sums, counts = evaluate(l, p, q, a, b)
            if k == 0:
                out["cost0"][p], out["n0"][p] = sums[EXPOSURE_COST], counts[0]
            lam, iters = float(s["lambda0"]), 0
            while True:
                x = exposure_step(sums, lam, estimate) if counts[0] >= min_pixels else None
                if x is None:
                    status = ALIGN_DEGENERATE
                    break
                if iters >= s["max_iters"]:
                    status = ALIGN_ITERATIONS
                    break
                trial, ta, tb = so3.mul(so3.exp(x[:3]), q), a + x[3], b + x[4]
                tsums, tcounts = evaluate(l, p, trial, ta, tb)
                iters += 1
                take = tcounts[0] >= min_pixels and tsums[EXPOSURE_COST] / tcounts[0] < sums[EXPOSURE_COST] / counts[0]
                if (estimate & EXPOSURE_GAIN) and not g_lo <= ta <= g_hi:
                    take = False
                if take:
                    q, a, b, sums, counts = trial, ta, tb, tsums, tcounts
                    out["last_x"][p] = x
                    lam = max(lam / s["lambda_down"], s["lambda_min"])
                    if np.linalg.norm(x[:3]) < s["tol_rot"]:
                        status = ALIGN_CONVERGED
                        break
                else:
                    lam *= s["lambda_up"]
                    if lam > s["lambda_max"]:
                        status = ALIGN_STALLED
                        break
            out["level_status"][p, k], out["level_iters"][p, k] = status, iters
            out["iters"][p] += iters
            out["q"][p], out["gain"][p], out["bias"][p], out["sums"][p], out["counts"][p], out["status"][p] = q, a, b, sums, counts, status
            if status == ALIGN_DEGENERATE:
                break
    out["info"] = pair_information(out["sums"][:, list(EXPOSURE_SHARED)], out["counts"])
    return out


def pair_candidates(q, status, window=1, min_gap=None, max_angle=0.0, max_per_frame=0):
    """The pairs (i, j), i < j, sorted, that a loop closure tries, from tracked rotations q [F, 4] and status [F] (io.TRACK_*; lost frames take no part): every
    pair of voting frames with j - i <= window, and, for |j - i| > min_gap (None: window), per frame the max_per_frame frames with the smallest rotation angle
    <= max_angle (rad) to it, ties to the lower index.  O(F^2) on the host; refused above PAIR_MAX_CANDIDATE_FRAMES frames."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 4)
    F = q.shape[0]
    if F > PAIR_MAX_CANDIDATE_FRAMES:
        raise ValueError(f"F = {F}: the candidate search is O(F^2) on the host and bounded at {PAIR_MAX_CANDIDATE_FRAMES} frames")
    st = np.asarray(status, dtype=np.int64).reshape(-1)
    if st.size != F:
        raise ValueError(f"status must be [{F}]")
    votes = (st == TRACK_ANCHOR) | (st == 2)
    gap = int(window) if min_gap is None else int(min_gap)
    out = set()
    idx = np.flatnonzero(votes)
    for i in idx:
        for j in idx[(idx > i) & (idx - i <= int(window))]:
            out.add((int(i), int(j)))
    if max_per_frame > 0 and idx.size:
        qn = q / np.linalg.norm(q, axis=1, keepdims=True)
        ang = 2.0 * np.arccos(np.clip(np.abs(qn @ qn.T), 0.0, 1.0))
        for i in idx:
            cand = idx[(np.abs(idx - i) > gap) & (ang[i, idx] <= float(max_angle))]
            order = cand[np.argsort(ang[i, cand], kind="stable")][:int(max_per_frame)]
            for j in order:
                out.add((int(min(i, j)), int(max(i, j))))
    return np.array(sorted(out), dtype=np.int32).reshape(-1, 2)


# ---- loop-closure pairs found by appearance (numpy forms of emba_frames_match_eval, emba_frames_match_search and emba_match_start, include/emba_hip.h; the
# device forms are LEGM.match_eval and LEGM.match_search, the host form LEGM.match_start).  The rule is emba_amd/csrc/match_rule.h's: the six
# sums of a shift are integers, the score's five operations are correctly rounded on both sides, so everything here has the device's bits.
MATCH_MAX_PIXELS = 16384                 # kMatchMaxPixels: a thumbnail
MATCH_MAX_PER_FRAME = 64                 # kMatchMaxPerFrame
MATCH_UNSCORED = -2.0                    # kMatchUnscored: the score of a pair without a scored shift
MATCH_SEARCH_MODES = ("rotations", "appearance", "both")


def match_check(sensor, level, rx, ry, n_min=1):
    """(w, h) of the thumbnails; the refusals of emba_frames_match_eval's level, range and n_min as ValueError, in its order."""
    sw, sh = int(sensor[0]), int(sensor[1])
    w, h = pair_level_size(sensor, level)
    if w * h > MATCH_MAX_PIXELS:
        l = next(l for l in range(64) if (sw >> l) * (sh >> l) <= MATCH_MAX_PIXELS)
        raise ValueError(f"level {int(level)} of a {sw} x {sh} sensor has {w} x {h} pixels: a thumbnail has {MATCH_MAX_PIXELS} at the most; the smallest level that fits is {l}")
    if not (0 <= int(rx) < w and 0 <= int(ry) < h):
        raise ValueError(f"rx = {rx}, ry = {ry}: 0 <= rx < {w} and 0 <= ry < {h} at level {int(level)}")
    if int(n_min) < 1:
        raise ValueError("n_min = 0: a scored shift has one pixel at the least")
    return w, h


def match_shifts(rx, ry):
    """The shifts (dx, dy) of a range, int64 [(2 rx + 1)(2 ry + 1), 2], row-major: dy from -ry, then dx from -rx."""
    dy, dx = np.meshgrid(np.arange(-int(ry), int(ry) + 1), np.arange(-int(rx), int(rx) + 1), indexing="ij")
    return np.stack([dx.ravel(), dy.ravel()], axis=1).astype(np.int64)


def _match_overlap(w, h, dx, dy):
    return max(-dx, 0), min(w - dx, w), max(-dy, 0), min(h - dy, h)


def match_sums(a_u8, b_u8, rx, ry, skip_zero=False):
    """The six integer sums of every shift of thumbnails a, b [h, w]: uint64 [shifts, 6] = n, sum a, sum b, sum a^2, sum b^2, sum a b over the overlap of
    A(x, y) with B(x + dx, y + dy); under skip_zero a point where either byte is 0 takes no part."""
    A, B = np.asarray(a_u8, dtype=np.uint8).astype(np.int64), np.asarray(b_u8, dtype=np.uint8).astype(np.int64)
    h, w = A.shape
    out = np.zeros((len(match_shifts(rx, ry)), 6), np.uint64)
    for s, (dx, dy) in enumerate(match_shifts(rx, ry)):
        x0, x1, y0, y1 = _match_overlap(w, h, int(dx), int(dy))
        if x1 <= x0 or y1 <= y0:
            continue
        a, b = A[y0:y1, x0:x1], B[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        m = ((a != 0) & (b != 0)) if skip_zero else np.ones(a.shape, bool)
        a, b = a[m], b[m]
        out[s] = (a.size, a.sum(), b.sum(), (a * a).sum(), (b * b).sum(), (a * b).sum())
    return out


def match_score(sums, n_min=1):
    """(score, scored) of sums [..., 6]: cov = n sab - sa sb, va = n saa - sa^2, vb likewise in int64; score = (double)cov |(double)cov| / ((double)va
    (double)vb), in this order; not scored (score MATCH_UNSCORED) where n < n_min, va = 0 or vb = 0."""
    s = np.asarray(sums).astype(np.int64)
    n, sa, sb, saa, sbb, sab = (s[..., k] for k in range(6))
    cov, va, vb = n * sab - sa * sb, n * saa - sa * sa, n * sbb - sb * sb
    scored = (n >= int(n_min)) & (va != 0) & (vb != 0)
    c = cov.astype(np.float64)
    den = np.where(scored, va.astype(np.float64) * vb.astype(np.float64), 1.0)
    return np.where(scored, (c * np.abs(c)) / den, MATCH_UNSCORED), scored


def match_best(a_u8, b_u8, rx, ry, skip_zero=False, n_min=1):
    """The best of a pair of thumbnails: the scored shift of greatest score, ties to the lowest shift index.  A dict of score, dx, dy, n, shift (the index)
    and sums [shifts, 6]; without a scored shift: MATCH_UNSCORED, (0, 0), 0."""
    sums = match_sums(a_u8, b_u8, rx, ry, skip_zero)
    score, scored = match_score(sums, n_min)
    if not scored.any():
        return dict(score=MATCH_UNSCORED, dx=0, dy=0, n=0, shift=0, sums=sums)
    s = int(np.argmax(np.where(scored, score, -np.inf)))      # (argmax: the first of equals)
    dx, dy = match_shifts(rx, ry)[s]
    return dict(score=float(score[s]), dx=int(dx), dy=int(dy), n=int(sums[s, 0]), shift=s, sums=sums)


def match_table(thumbs_u8, rx, ry, skip_zero=False, n_min=1):
    """The best of every ordered pair (i, j) of thumbnails [F, h, w] at once: score [F, F] (MATCH_UNSCORED: none), shift int64 [F, F, 2], n int64 [F, F].  The
    sums of a shift are matrix products over the overlap, taken in fp64 where every partial sum is an integer below 2^53: exact in any order."""
    T = np.asarray(thumbs_u8, dtype=np.uint8)
    F, h, w = T.shape
    best, have = np.full((F, F), MATCH_UNSCORED), np.zeros((F, F), bool)
    bshift, bn = np.zeros((F, F, 2), np.int64), np.zeros((F, F), np.int64)
    for dx, dy in match_shifts(rx, ry):
        dx, dy = int(dx), int(dy)
        x0, x1, y0, y1 = _match_overlap(w, h, dx, dy)
        if x1 <= x0 or y1 <= y0:
            continue
        A = T[:, y0:y1, x0:x1].reshape(F, -1).astype(np.float64)
        B = T[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx].reshape(F, -1).astype(np.float64)
        Ma, Mb = ((A != 0).astype(np.float64), (B != 0).astype(np.float64)) if skip_zero else (np.ones_like(A), np.ones_like(B))
        sums = np.stack([Ma @ Mb.T, A @ Mb.T, Ma @ B.T, (A * A) @ Mb.T, Ma @ (B * B).T, A @ B.T], axis=-1).astype(np.int64)
        score, scored = match_score(sums, n_min)
        take = scored & (~have | (score > best))      # (the shifts come in index order: an equal score stays with the lower index)
        best, have = np.where(take, score, best), have | take
        bshift[take], bn[take] = (dx, dy), sums[..., 0][take]
    return best, bshift, bn


def match_search(frames_u8, status=None, level=0, rx=0, ry=0, min_gap=0, skip_zero=False, n_min=1, score_min=0.0, k=1):
    """emba_frames_match_search in numpy: frames_u8 [F, sh, sw]; the thumbnails are pair_level_bytes of `level`; candidates are i < j with j - i > min_gap,
    both frames voting (status [F] of TRACK_*: anchor or tracked; None: all); per frame the k partners of greatest best score >= score_min, ties to the lower
    partner index.  A dict of partner int32 [F, k] (-1), score [F, k] (MATCH_UNSCORED), shift int32 [F, k, 2] (from the lower index to the higher), n int64
    [F, k]."""
    fr = np.asarray(frames_u8, dtype=np.uint8)
    F, sh, sw = fr.shape
    match_check((sw, sh), level, rx, ry, n_min)
    k, gap = int(k), int(min_gap)
    if not 1 <= k <= MATCH_MAX_PER_FRAME or gap < 0 or np.isnan(score_min):
        raise ValueError(f"k = {k} (1 ... {MATCH_MAX_PER_FRAME}), min_gap = {gap} (not negative), score_min = {score_min} (a number)")
    st = np.full(F, TRACK_ANCHOR, np.int64) if status is None else np.asarray(status, dtype=np.int64).reshape(-1)
    votes = (st == TRACK_ANCHOR) | (st == 2)
    best, bshift, bn = match_table(pair_level_bytes(fr, level, skip_zero), rx, ry, skip_zero, n_min)
    iu = np.triu(np.ones((F, F), bool), 1)      # (i < j as evaluated, mirrored: the partner's side keeps the orientation)
    best, bn = np.where(iu, best, best.T), np.where(iu, bn, bn.T)
    bshift = np.where(iu[..., None], bshift, bshift.transpose(1, 0, 2))
    idx = np.arange(F)
    ok = votes[:, None] & votes[None, :] & (np.abs(idx[:, None] - idx[None, :]) > gap) & (bn > 0) & (best >= float(score_min))
    out = dict(partner=np.full((F, k), -1, np.int32), score=np.full((F, k), MATCH_UNSCORED), shift=np.zeros((F, k, 2), np.int32), n=np.zeros((F, k), np.int64))
    for f in range(F):
        g = np.flatnonzero(ok[f])
        g = g[np.lexsort((g, -best[f, g]))][:k]
        out["partner"][f, :g.size], out["score"][f, :g.size], out["shift"][f, :g.size], out["n"][f, :g.size] = g, best[f, g], bshift[f, g], bn[f, g]
    return out


def match_pairs(found, with_info=False):
    """The pairs (i, j), i < j, int32 [P, 2], sorted: the union of the per-frame lists of match_search / LEGM.match_search.  with_info: also score [P] and
    shift int32 [P, 2] of each."""
    seen = {}
    for f, row in enumerate(np.asarray(found["partner"])):
        for t, g in enumerate(row):
            if g >= 0:
                seen[(min(f, int(g)), max(f, int(g)))] = (float(found["score"][f, t]), tuple(int(v) for v in found["shift"][f, t]))
    keys = sorted(seen)
    pairs = np.array(keys, dtype=np.int32).reshape(-1, 2)
    if not with_info:
        return pairs
    return pairs, np.array([seen[p][0] for p in keys], dtype=np.float64), np.array([seen[p][1] for p in keys], dtype=np.int32).reshape(-1, 2)


def match_start(dx, dy, level, fu, fv, cu, cv, sw, sh):
    """emba_match_start in Python floats (IEEE doubles; + - * / sqrt in match_rule.h's order, so the same bits): xyzw [4] of the shortest arc from the pinhole
    bearing of p_i = c - t to that of p_j = c + t, c = ((sw - 1) / 2, (sh - 1) / 2), t = 2^l (dx, dy) / 2.  R(Q) b_i = b_j: pair_start's convention."""
    import math
    l = int(level)
    fu, fv, cu, cv = float(fu), float(fv), float(cu), float(cv)
    if not (0 <= l <= PAIR_MAX_LEVEL and int(sw) > 0 and int(sh) > 0 and math.isfinite(fu) and math.isfinite(fv) and fu > 0.0 and fv > 0.0 and math.isfinite(cu)
            and math.isfinite(cv)):
        raise ValueError("match_start: a level 0 ... 7, a sensor with pixels, fu and fv finite and positive, cu and cv finite")
    cx, cy = (float(int(sw)) - 1.0) / 2.0, (float(int(sh)) - 1.0) / 2.0
    tx, ty = float(1 << l) * float(int(dx)) / 2.0, float(1 << l) * float(int(dy)) / 2.0

    def bearing(x, y):
        bx, by = (x - cu) / fu, (y - cv) / fv
        n = math.sqrt((bx * bx + by * by) + 1.0)
        return bx / n, by / n, 1.0 / n

    bi, bj = bearing(cx - tx, cy - ty), bearing(cx + tx, cy + ty)
    x, y, z = bi[1] * bj[2] - bi[2] * bj[1], bi[2] * bj[0] - bi[0] * bj[2], bi[0] * bj[1] - bi[1] * bj[0]
    w = 1.0 + ((bi[0] * bj[0] + bi[1] * bj[1]) + bi[2] * bj[2])
    n = math.sqrt(((x * x + y * y) + z * z) + w * w)
    return np.array([x / n, y / n, z / n, w / n])


def graph_settings(**kw):
    """GRAPH_DEFAULTS with the given members replaced; the refusals of emba_rotation_graph_solve's settings as ValueError."""
    unknown = set(kw) - set(GRAPH_DEFAULTS)
    if unknown:
        raise ValueError(f"unknown settings {sorted(unknown)}")
    s = dict(GRAPH_DEFAULTS, **kw)
    ok = (int(s["max_iters"]) >= 0 and int(s["cg_max_iters"]) >= 1 and np.isfinite(s["lambda0"]) and s["lambda0"] > 0.0 and np.isfinite(s["lambda_up"])
          and np.isfinite(s["lambda_down"]) and s["lambda_up"] > 1.0 and s["lambda_down"] > 1.0 and 0.0 <= s["lambda_min"] <= s["lambda_max"]
          and s["lambda_max"] > 0.0 and s["tol"] >= 0.0 and s["cg_tol"] >= 0.0)
    if not ok:
        raise ValueError(f"settings out of range: {s}")
    return s


def graph_log(q):
    """The rotation vector of the shorter way round of the quaternion q (xyzw): graph_qlog."""
    q = np.asarray(q, dtype=np.float64)
    q = -q if q[3] < 0.0 else q
    n2 = float(q[:3] @ q[:3])
    if n2 < 1e-20:
        f = 2.0 / q[3] - (2.0 / 3.0) * n2 / q[3] ** 3
    else:
        n = np.sqrt(n2)
        f = 2.0 * np.arctan2(n, q[3]) / n
    return f * q[:3]


def graph_jr_inv(e):
    """Jr^-1(e) = I + [e]x / 2 + c [e]x^2, c = (1 - (th / 2) cot(th / 2)) / th^2: graph_jr_inv."""
    e = np.asarray(e, dtype=np.float64)
    th2 = float(e @ e)
    if th2 < 1e-8:
        c = 1.0 / 12.0 + th2 / 720.0
    else:
        th = np.sqrt(th2)
        c = (1.0 - 0.5 * th * np.cos(0.5 * th) / np.sin(0.5 * th)) / th2
    K = np.array([[0.0, -e[2], e[1]], [e[2], 0.0, -e[0]], [-e[1], e[0], 0.0]])
    return np.eye(3) + 0.5 * K + c * (K @ K)


def _graph_info(info6):
    a = np.asarray(info6, dtype=np.float64)
    return np.array([[a[0], a[1], a[2]], [a[1], a[3], a[4]], [a[2], a[4], a[5]]])


def graph_residual(Qij, qi, qj):
    """e = log(Q_ij (x) q_i^-1 (x) q_j)."""
    return graph_log(so3.mul(so3.mul(Qij, so3.inverse(qi)), qj))


def rotation_graph_solve(q_xyzw, status, edges, Q_xyzw, info, **settings):
    """emba_rotation_graph_solve in numpy (graph_rule.h): the anchors of status (TRACK_ANCHOR) held exactly, damped Gauss-Newton with the linear system
    assembled densely and solved directly, where the C form runs preconditioned conjugate gradients to cg_tol: the two agree to that tolerance.  A dict of q,
    cost0, cost, iters, end.  The refusals are graph_args_ok's, in its order, as ValueError: the settings, a q that is not finite or of zero norm, no anchor,
    an edge out of range, an edge's Q not finite or of zero norm, an info that is not finite, the first unreachable frame (named in the message)."""
    from . import synth
    s = graph_settings(**settings)
    q = np.array(q_xyzw, dtype=np.float64).reshape(-1, 4)
    st = np.asarray(status, dtype=np.int64).reshape(-1)
    F = q.shape[0]
    ed = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    E = ed.shape[0]
    Qe = np.asarray(Q_xyzw, dtype=np.float64).reshape(E, 4)
    Lam = np.asarray(info, dtype=np.float64).reshape(E, 6)
    def first_bad(quats):      # the first quaternion that is not finite or has zero norm (align_q_ok), None where there is none
        n2 = (quats * quats).sum(axis=1)
        bad = np.flatnonzero(~(np.isfinite(n2) & (n2 > 0.0)))
        return int(bad[0]) if bad.size else None

    if st.size != F:
        raise ValueError(f"status must be [{F}]")
    if first_bad(q) is not None:      # (the refusals in graph_args_ok's order)
        raise ValueError(f"q_xyzw[{first_bad(q)}] is not finite or has zero norm")
    if not (st == TRACK_ANCHOR).any():
        raise ValueError("no anchor: a rotation graph needs a frame that is held")
    if E and (ed.min() < 0 or ed.max() >= F):
        raise ValueError("an edge names a frame outside [0, F)")
    if first_bad(Qe) is not None:
        raise ValueError(f"Q_xyzw[{first_bad(Qe)}] is not finite or has zero norm")
    if not np.isfinite(Lam).all():
        raise ValueError("an info is not finite")
    reached = st == TRACK_ANCHOR
    grew = True
    while grew:
        grew = False
        for i, j in ed:
            if reached[i] != reached[j]:
                reached[i] = reached[j] = True
                grew = True
    touched = np.zeros(F, bool)
    touched[ed.reshape(-1)] = True
    bad = np.flatnonzero(touched & ~reached)
    if bad.size:
        raise ValueError(f"frame {int(bad[0])} is named by an edge, but no path of edges leads from an anchor to it")
    free = touched & (st != TRACK_ANCHOR)

    def cost_of(qq):
        return float(sum(e @ _graph_info(Lam[k]) @ e for k in range(E) for e in [graph_residual(Qe[k], qq[ed[k, 0]], qq[ed[k, 1]])]))

    q_in = q.copy()
    cost0 = cost = cost_of(q)
    out = dict(q=q_in.copy(), cost0=cost0, cost=cost, iters=0, end=GRAPH_CONVERGED)
    if not free.any():
        return out
    lam, iters, end = float(s["lambda0"]), 0, GRAPH_ITERATIONS
    col = -np.ones(F, np.int64)
    col[free] = np.arange(int(free.sum()))
    n = 3 * int(free.sum())
    while iters < s["max_iters"]:
        A, g = np.zeros((n, n)), np.zeros(n)
        for k in range(E):
            i, j = ed[k]
            if i == j:
                continue
            e = graph_residual(Qe[k], q[i], q[j])
            M = graph_jr_inv(e) @ synth._quat_to_R(q[j]).T
            L = _graph_info(Lam[k])
            W, ge = M.T @ L @ M, M.T @ (L @ e)
            for a_, sa in ((i, -1.0), (j, 1.0)):
                if col[a_] < 0:
                    continue
                ra = slice(3 * col[a_], 3 * col[a_] + 3)
                g[ra] += sa * ge
                for b_, sb in ((i, -1.0), (j, 1.0)):
                    if col[b_] >= 0:
                        A[ra, 3 * col[b_]:3 * col[b_] + 3] += sa * sb * W
        try:
            x = np.linalg.solve(A + lam * np.diag(np.diag(A)), -g)
        except np.linalg.LinAlgError:
            end = GRAPH_DEGENERATE
            break
        trial = q.copy()
        for f in np.flatnonzero(free):
            trial[f] = so3.mul(so3.exp(x[3 * col[f]:3 * col[f] + 3]), q[f])
        c1 = cost_of(trial)
        iters += 1
        dmax = float(np.abs(x).max())
        if c1 < cost:
            q, cost = trial, c1
            lam = max(lam / s["lambda_down"], s["lambda_min"])
            if dmax < s["tol"]:
                end = GRAPH_CONVERGED
                break
        else:
            if dmax < s["tol"]:
                end = GRAPH_CONVERGED
                break
            lam *= s["lambda_up"]
            if lam > s["lambda_max"]:
                end = GRAPH_STALLED
                break
    q[~free] = q_in[~free]
    return dict(q=q, cost0=cost0, cost=cost, iters=iters, end=end)
