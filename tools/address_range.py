"""Lane and frame tiling, and the sizes at the edges of the kernels' 32-bit address range (tests/test_address_range_cpu.py,
tests/test_gpu_address_range.py).

All arithmetic of the library is columnwise over GF(256): output byte lane s of a frame depends on input lane s only, and a frame
on no other frame.  A problem with a huge symbol length S is therefore checked on every byte at the price of a small one: the small
problem has P lanes, the big input is small[..., s mod P] for s < S (the last tile may be ragged), and the big output must be the
small output tiled the same way.  P = 4080 = 16 * 255 is odd times 16, so no power of two is a multiple of P: an access displaced by
2^24, 2^31, 2^32 (or any other power of two from 16 up) lands on a lane of different content, and a wrong row on another row.  The
batch axis is tiled alike with a prime period: frame f of the big batch is frame f mod PF of the small one.

Nothing here imports the library or the oracle: numpy always, torch only inside the functions that take torch tensors."""
import numpy as np

P = 4080      # lanes of the small problem
PF = 7        # frames of the small problem on the batch axis (prime)

# The limits of the kernels ("Address range")
LIM_OFFSET = 1 << 32      # bytes a frame's 32-bit offsets reach: n * S (rows), n * (8 + S) (packets), stride * (8 + S) (flows)
LIM_SIGN = 1 << 31        # no limit of the library: the first offset with bit 31 set
LIM_MUL24 = 1 << 24       # an operand of the 24-bit multiply: S, 8 + S
LIM_RS_ROW = 1 << 23      # RS decode from frames: idx * S with idx < 256 in 32 bits


# ------------------------------------------------------------------------------------------------ edge sizes
def last_below(limit, rows=1, extra=0, unit=256):
    """The largest multiple S of `unit` with rows * (extra + S) < limit."""
    s = ((limit - 1) // rows - extra) // unit * unit
    assert s > 0 and rows * (extra + s) < limit <= rows * (extra + s + unit)
    return s


def first_from(limit, rows=1, extra=0, unit=256):
    """The smallest multiple S of `unit` with rows * (extra + S) >= limit."""
    return last_below(limit, rows, extra, unit) + unit


def edge_pair(limit, rows=1, extra=0, unit=256):
    return last_below(limit, rows, extra, unit), first_from(limit, rows, extra, unit)


def word_size_above(limit, rows=1, unit=256):
    """A word-form S beyond the limit: a multiple of 4 that is no multiple of 16, 20 bytes past the first multiple of `unit`."""
    s = first_from(limit, rows, 0, unit) + 20
    assert s % 4 == 0 and s % 16 != 0 and rows * s >= limit
    return s


def frames_from(limit, frame_bytes):
    """The smallest number of frames F with F * frame_bytes >= limit + frame_bytes: the last frame STARTS at or beyond the limit."""
    f = -(-limit // frame_bytes) + 1
    assert (f - 1) * frame_bytes >= limit > (f - 2) * frame_bytes
    return f


def stride_pair(S, limit=LIM_OFFSET):
    """The multi-flow sender's stride (packets) with stride * (8 + S) on either side of the limit."""
    lo = (limit - 1) // (8 + S)
    assert lo * (8 + S) < limit <= (lo + 1) * (8 + S)
    return lo, lo + 1


# ------------------------------------------------------------------------------------------------ tiling, numpy
def tile_lanes(small, S, period=P):
    """small [..., period] -> [..., S] with out[..., s] = small[..., s mod period]."""
    assert small.shape[-1] == period
    reps = -(-S // period)
    return np.ascontiguousarray(np.tile(small, (1,) * (small.ndim - 1) + (reps,))[..., :S])


def tile_frames(small, F):
    """small [PF, ...] -> [F, ...] with out[f] = small[f mod PF]."""
    pf = small.shape[0]
    return np.ascontiguousarray(small[np.arange(F) % pf])


def lanes_equal(big, small, period=P):
    """Is big [..., S] the lane tiling of small [..., period]?  Tile by tile."""
    S = big.shape[-1]
    if big.shape[:-1] != small.shape[:-1] or small.shape[-1] != period:
        return False
    for t0 in range(0, S, period):
        w = min(period, S - t0)
        if not np.array_equal(big[..., t0:t0 + w], small[..., :w]):
            return False
    return True


# ------------------------------------------------------------------------------------------------ tiling, torch (device)
_CHUNK = 192 << 20   # bytes one comparison may take for its temporary


def fill_lanes(big, small):
    """big [..., S] (a view into device memory, last axis contiguous) <- the lane tiling of small [..., period].  No temporary."""
    period, S = small.shape[-1], big.shape[-1]
    full = S // period
    if full:
        big[..., :full * period].unflatten(-1, (full, period)).copy_(small.unsqueeze(-2).expand(*small.shape[:-1], full, period))
    if S > full * period:
        big[..., full * period:].copy_(small[..., :S - full * period])
    return big


def fill_frames(big, small):
    """big [F, ...] <- small[f mod PF]."""
    pf, F = small.shape[0], big.shape[0]
    full = F // pf
    if full:
        big[:full * pf].unflatten(0, (full, pf)).copy_(small.unsqueeze(0).expand(full, *small.shape))
    if F > full * pf:
        big[full * pf:].copy_(small[:F - full * pf])
    return big


def lanes_mismatch(big, small):
    """The first (leading index..., tile) at which big [..., S] is not the lane tiling of small [..., period], or None.  Every byte
    is compared, groups of tiles at a time so that the temporary stays small; one read-back at the end."""
    import torch
    period, S = small.shape[-1], big.shape[-1]
    assert tuple(big.shape[:-1]) == tuple(small.shape[:-1])
    lead = int(np.prod(small.shape[:-1])) if small.ndim > 1 else 1
    full = S // period
    group = max(1, _CHUNK // max(1, lead * period))
    bad = torch.zeros((), dtype=torch.bool, device=big.device)
    want = small.unsqueeze(-2)
    for t0 in range(0, full, group):
        t1 = min(full, t0 + group)
        bad |= (big[..., t0 * period:t1 * period].unflatten(-1, (t1 - t0, period)) != want).any()
    if S > full * period:
        bad |= (big[..., full * period:] != small[..., :S - full * period]).any()
    if not bool(bad):
        return None
    # slow path, only to name the place
    for t in range(-(-S // period)):
        w = min(period, S - t * period)
        ne = big[..., t * period:t * period + w] != small[..., :w]
        if bool(ne.any()):
            idx = torch.nonzero(ne)[0].tolist()
            return tuple(idx[:-1]) + (t, idx[-1])
    return ("?",)


def frames_mismatch(big, small):
    """The first frame f with big[f] != small[f mod PF], or None."""
    import torch
    pf, F = small.shape[0], big.shape[0]
    per = max(1, int(np.prod(small.shape[1:])))
    group = max(1, _CHUNK // (pf * per))
    full = F // pf
    bad = []
    for q0 in range(0, full, group):
        q1 = min(full, q0 + group)
        ne = (big[q0 * pf:q1 * pf].unflatten(0, (q1 - q0, pf)) != small.unsqueeze(0)).flatten(2).any(-1) if small.ndim > 1 else \
            (big[q0 * pf:q1 * pf].unflatten(0, (q1 - q0, pf)) != small.unsqueeze(0))
        nz = torch.nonzero(ne.reshape(-1))
        if nz.numel():
            bad.append(q0 * pf + int(nz[0]))
            break
    if not bad and F > full * pf:
        ne = big[full * pf:] != small[:F - full * pf]
        ne = ne.flatten(1).any(-1) if small.ndim > 1 else ne
        nz = torch.nonzero(ne)
        if nz.numel():
            bad.append(full * pf + int(nz[0]))
    return bad[0] if bad else None
