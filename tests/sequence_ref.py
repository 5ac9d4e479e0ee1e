"""Independent restatements of the sequence-level steps of the reference's EMBA::EMBA / EMBA::Run (src/emba/emba.cpp), written from that file
loop for loop — nothing here imports emba_amd.  What tests/test_sequence_cpu.py and tests/test_gpu_sequence.py compare the numpy and the device
forms with."""
import numpy as np

SIZE_MAX = (1 << 64) - 1


class NoEvents(Exception):
    """The reference's subset is not a valid range here: `idx_ev_subset_end -= 100` underflowed size_t, or end < beg."""


def downsample(x, y, pol, t, rate):
    """emba.cpp:281-304, the counting loop as written."""
    if rate < 2:
        return x, y, pol, t
    keep = []
    sampling_count = 1
    for i in range(len(t)):
        if sampling_count == rate:
            keep.append(i)
            sampling_count = 1
        else:
            sampling_count += 1
    keep = np.array(keep, dtype=np.int64)
    return x[keep], y[keep], pol[keep], t[keep]


def event_subset(t, t_beg_ns, t_end_ns):
    """emba.cpp:473-510, the two probing loops as written (size_t arithmetic made explicit)."""
    n = len(t)
    a = t_beg_ns + 1_000_000         # t_beg + ros::Duration(1e-3)
    b = t_end_ns - 1_000_000
    beg = 0
    while beg < n:
        if t[beg] > a:
            break
        beg += 100
    end = beg
    while end < n:
        if t[end] > b:
            end = (end - 100) & SIZE_MAX
            break
        end += 100
    if end > SIZE_MAX // 2:
        raise NoEvents("the tail cursor underflowed")
    if end > n:
        end = n
    if end < beg:
        raise NoEvents("reversed range")
    return beg, end


def median_blur3(plane):
    """emba.cpp:357-364 for one plane, pixel by pixel: float32 copy, the median of the 3x3 neighbourhood with coordinates clamped to the image
    (BORDER_REPLICATE), back to float64."""
    a = np.asarray(plane, dtype=np.float64).astype(np.float32)
    h, w = a.shape
    out = np.empty((h, w), dtype=np.float64)
    for r in range(h):
        rows = [min(max(r + d, 0), h - 1) for d in (-1, 0, 1)]
        for c in range(w):
            cols = [min(max(c + d, 0), w - 1) for d in (-1, 0, 1)]
            vals = sorted(float(a[i, j]) for i in rows for j in cols)
            out[r, c] = vals[4]
    return out


def median_blur3_fast(plane):
    """The same for planes too large for the pixel loop: nine shifted copies, sorted (checked against median_blur3 in test_sequence_cpu.py)."""
    a = np.asarray(plane, dtype=np.float64).astype(np.float32)
    h, w = a.shape
    ri = np.clip(np.arange(-1, h + 1), 0, h - 1)
    ci = np.clip(np.arange(-1, w + 1), 0, w - 1)
    p = a[np.ix_(ri, ci)]
    nine = np.stack([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)])
    nine.sort(axis=0)
    return nine[4].astype(np.float64)
