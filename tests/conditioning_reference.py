"""TEST INFRASTRUCTURE: a plain restatement of what the resampler does to the taught points before its first arc-length pass
(include/batotp_hip.h, the block around struct batotp_resample_params): close-point removal, the stretch of two or three survivors
onto four points, input smoothing -> decimation -> smoothing, and the checksum the stage trace keeps of the result.

Written from the documented behaviour on Python floats (IEEE fp64), one operation per statement, so that no compiler decides
anything; independent of the C oracle, which the tests compare it with (tests/test_conditioning_cpu.py) before the device is
compared with both (tests/test_gpu_taught_conditioning.py).  Rows are lists of floats, channel-major: x[channel][point]."""
import math
import struct

TOO_SHORT = 1     # BATOTP_RS_TOO_SHORT
MASK = (1 << 64) - 1


def _step_sq(x, rows, i):
    """squared distance between points i - 1 and i over the driving rows, summed in row order"""
    total = 0.0
    for c in rows:
        d = x[c][i] - x[c][i - 1]
        sq = d * d
        total = total + sq
    return total


def remove_close_points(x, rows, thresh):
    """Drop every point closer than `thresh` (strictly) to its predecessor, unless that predecessor was itself dropped in the
    same round; never the last point: when it would go, the one before it goes instead and the one before that stays.  Rounds
    repeat on the survivors until one drops nothing.  Returns new rows."""
    x = [list(r) for r in x]
    limit = thresh * thresh
    while True:
        n = len(x[0])
        drop = [False] * n
        found = False
        for i in range(1, n):
            if _step_sq(x, rows, i) < limit and not drop[i - 1]:
                drop[i] = True
                found = True
        if drop[n - 1] and n > 2:
            drop[n - 1] = False
            drop[n - 2] = True
            drop[n - 3] = False
        if not found:
            return x
        x = [[v for v, gone in zip(r, drop) if not gone] for r in x]


def stretch_to_four(x, sres):
    """two or three points onto four evenly spaced ones by linear interpolation over the normalised index; the spacing grows
    by (n - 1) / 3"""
    n = len(x[0])
    step_old = 1.0 / float(n - 1)
    step_new = 1.0 / 3.0
    at_old = [step_old * float(k) for k in range(n)]
    at_new = [step_new * float(k) for k in range(4)]
    out = [[0.0] * 4 for _ in x]
    seg = 0
    for i in range(4):
        while not (at_new[i] < at_old[seg + 1] or seg == n - 2):
            seg += 1
        num = at_new[i] - at_old[seg]
        den = at_old[seg + 1] - at_old[seg]
        tau = num / den
        for c, r in enumerate(x):
            rise = r[seg + 1] - r[seg]
            part = rise * tau
            out[c][i] = r[seg] + part
    scaled = sres * float(n - 1)
    return out, scaled / 3.0


def smooth_row(r, window):
    """centred moving average.  The window is clamped to the length and made odd downwards (half width w/2 + w%2 - 1); the end
    points stay; next to the ends the window shrinks to what fits symmetrically, summed from the end inwards"""
    n = len(r)
    w = min(window, n)
    half = w // 2 + w % 2 - 1
    w = 2 * half + 1
    out = list(r)
    for i in range(1, n - 1):
        if i < half:
            span = 2 * i + 1
            acc = 0.0
            for j in range(span):
                acc = acc + r[j]
            out[i] = acc / span
        elif i >= n - half:
            span = 2 * (n - 1 - i) + 1
            acc = 0.0
            for j in range(span):
                acc = acc + r[n - 1 - j]
            out[i] = acc / span
        else:
            acc = 0.0
            for j in range(i - half, i + half + 1):
                acc = acc + r[j]
            out[i] = acc / w
    return out


def decimate_row(r, fact):
    """every fact-th sample; the last sample always ends the row (it replaces the last regular one unless that IS the last)"""
    n = len(r)
    n_out = (n - 1) // fact + 1
    out = [r[fact * i] for i in range(n_out)]
    if fact * (n_out - 1) + 1 != n:
        out[n_out - 1] = r[n - 1]
    return out


def condition(x, sres, rows, thresh, decim, smooth_window):
    """x[C][n], spacing sres, driving rows `rows` (a range) -> (x'[C][n'], sres', status).  A non-zero status means the path
    is refused; x' is then whatever was reached."""
    rows = list(rows)
    x = remove_close_points([[float(v) for v in r] for r in x], rows, thresh)
    n = len(x[0])
    if n < 2:
        return x, sres, TOO_SHORT
    if n < 4:
        x, sres = stretch_to_four(x, sres)
    fact = decim if decim > 1 else 1
    if fact > 1 or smooth_window > 1:
        if fact > 1:
            for c in rows:
                x[c] = smooth_row(x[c], fact)
            x = [decimate_row(r, fact) for r in x]
            sres = sres * fact
        if smooth_window > 1:
            for c in rows:
                x[c] = smooth_row(x[c], fact)     # the decimation factor is the window of BOTH smoothing passes
        if len(x[0]) < 4:
            return x, sres, TOO_SHORT
    return x, sres, 0


def cable_lengths(x, n_joints, pmat):
    """the joint rows of the cable robot from the platform position (rows n_joints .. n_joints + 2): the distance to each cable's
    exit point, pmat row-major 3 x 3 with one exit point per COLUMN; x, y, z squares added in that order"""
    x = [list(r) for r in x]
    for i in range(len(x[0])):
        for k in range(3):
            dx = x[n_joints + 0][i] - pmat[0 * 3 + k]
            dy = x[n_joints + 1][i] - pmat[1 * 3 + k]
            dz = x[n_joints + 2][i] - pmat[2 * 3 + k]
            xx = dx * dx
            yy = dy * dy
            zz = dz * dz
            sq = 0.0 + xx
            sq = sq + yy
            sq = sq + zz
            x[k][i] = math.sqrt(sq)
    return x


def _mix64(v):
    """the splitmix64 finaliser"""
    v ^= v >> 30
    v = (v * 0xBF58476D1CE4E5B9) & MASK
    v ^= v >> 27
    v = (v * 0x94D049BB133111EB) & MASK
    return v ^ (v >> 31)


def stage_checksum(x):
    """wrap-around sum over the values, row after row, of mix64(bits XOR (index + 1) * 0x9E3779B97F4A7C15)"""
    total = 0
    index = 0
    for r in x:
        for v in r:
            index += 1
            bits = struct.unpack("<Q", struct.pack("<d", float(v)))[0]
            total = (total + _mix64(bits ^ ((index * 0x9E3779B97F4A7C15) & MASK))) & MASK
    return total
