"""Guarded buffers: what a kernel or collective call touches besides its result.

The GPU suite pins what every entry point computes inside [out, out + n).  tests/test_gpu_footprint.py also pins
what else a call writes: every output sits between two guard bands and every input is compared, guards and payload,
with a snapshot taken before the call.

Layout.  A Guarded is ONE torch.uint8 allocation: lower guard, payload, upper guard.  The payload's address is
`phase` (0..15) bytes past a 16-byte boundary, so a test chooses the scalar head `align_split` cuts.  The whole
allocation is first stamped with position-dependent pseudo-random bytes (splitmix64 of the key and the 8-byte word
index); load() then overwrites the payload.  A stray store of an operand, of a result or of a constant cannot
reproduce the stamp, so any write outside the payload shows as differing bytes.  Nothing is ever placed at the end of
an allocation to catch an overrun by faulting: an overrun of up to the guard's size lands in memory the test owns
and is reported with its offset.  Out-of-bounds READS that do not change a result are out of scope: no guard can see
them.

Guard size.  GUARD_BYTES is four times the largest trip (workgroup size x vectors per lane x 16 bytes) of any
compiled kernel shape, TRIP_SHAPES below, taken from the kernels' own constants:
  bucket kernel  (csrc/reduce_vec.hpp: kBlock = 256 threads plain, 64 streaming; vec_u <= 4)            16 KiB
  tree kernel    (csrc/reduce_tree.hpp: the same workgroups; tree_u <= 4)                                16 KiB
  user-op fold   (include/chiara_user_op.hpp launch_fold: block = 256, CHR_USER_FOLD_U = 4)              16 KiB
  user-op tree   (include/chiara_user_op.hpp: kTreeBlock = 64, tree_u <= 4)                               4 KiB
so 64 KiB on each side: a kernel that runs one whole trip, or one grid-stride round of the scalar kernels' 256
lanes, past either end of its range still lands inside the guard.  tests/test_footprint_util.py reads the constants
back out of the sources, so the table cannot go stale unnoticed.
Streaming launches go through the XCD map with the odd-XCD handover (reduce_common.hpp xcd_trip_w): their grids hold
`trips + 8 * hand` workgroups with hand <= trips / 16, and the surplus workgroups must idle.  Everything they could
address lies within (grid - trips) x trip bytes <= half the payload past its end; stream_guard(nbytes) -- the
payload's own size, at least GUARD_BYTES -- covers it.

Checks run on the tensor's own device (torch.equal, then != and nonzero only where something differs); no guard is
copied to the host.  The class works on CPU tensors too (device="cpu"), which is how its own tests show that every
check can fail."""
import numpy as np
import torch

# (threads per workgroup, 16-byte vectors per lane per trip) of every compiled shape, largest U of each
TRIP_SHAPES = {
    "bucket plain": (256, 4),      # reduce_vec.hpp launch_vec_m: BL = 256, vec_u<M, false> = 4 (m <= 2) or 2
    "bucket streaming": (64, 4),   # BL = 64, vec_u_nt = 4 (m = 1), 2, 1
    "tree plain": (256, 4),        # reduce_tree.hpp launch_tree_nl: BL = 256, tree_u<NL, false> = 4 (<= 4 leaves) or 2
    "tree streaming": (64, 4),     # BL = 64, tree_u<NL, true> = 4 (2 leaves), 2, 1
    "user fold": (256, 4),         # chiara_user_op.hpp launch_fold: block = 256, kU = CHR_USER_FOLD_U = 4
    "user tree": (64, 4),          # chiara_user_op.hpp: kTreeBlock = 64, tree_u<NL> = 4 (2 leaves), 2, 1
}
MAX_TRIP_BYTES = max(bl * u * 16 for bl, u in TRIP_SHAPES.values())
GUARD_BYTES = 4 * MAX_TRIP_BYTES
assert GUARD_BYTES >= 64 << 10


def stream_guard(nbytes):
    """Upper guard for a payload that goes through the XCD map and the handover: the payload's own size."""
    return max(int(nbytes), GUARD_BYTES)


def _stamp(key, nbytes):
    """nbytes position-dependent bytes: the little-endian bytes of splitmix64(key-mix + word index)."""
    nw = (nbytes + 7) // 8
    with np.errstate(over="ignore"):
        x = np.arange(nw, dtype=np.uint64) + np.uint64((int(key) * 0xD1342543DE82EF95 + 0x2545F4914F6CDD1D) % (1 << 64))
        x += np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x.view(np.uint8)[:nbytes]


class Diff(tuple):
    """(region, offset, count): `count` bytes differ in `region` ("lower", "payload" or "upper"), the first of them
    `offset` bytes from the payload's start (negative in the lower guard)."""
    __slots__ = ()

    def __new__(cls, region, offset, count):
        return super().__new__(cls, (region, int(offset), int(count)))

    region = property(lambda s: s[0])
    offset = property(lambda s: s[1])
    count = property(lambda s: s[2])


class Check:
    """The outcome of guards_intact() / unchanged_since(): true when nothing differs, else .diffs lists one Diff per
    region that does; str() names them for an assertion message."""

    def __init__(self, diffs, what=""):
        self.diffs = list(diffs)
        self.what = what

    def __bool__(self):
        return not self.diffs

    def __eq__(self, other):
        return self.diffs == (other.diffs if isinstance(other, Check) else other)

    def __repr__(self):
        if not self.diffs:
            return f"{self.what}: intact"
        return f"{self.what}: " + "; ".join(f"{d.count} byte(s) differ in the {d.region} region from payload offset "
                                             f"{d.offset:+d}" for d in self.diffs)


class Guarded:
    """`nbytes` of payload, `phase` bytes past a 16-byte boundary, between guards of at least `lo_guard` and
    `hi_guard` stamped bytes, in one allocation on `device` (default: the GPU).  `capacity` >= nbytes reserves room
    so that reset(nbytes) can re-stamp the allocation and move the payload's end: one allocation then serves a whole
    sweep of sizes at one phase, the upper guard growing as the payload shrinks."""

    def __init__(self, nbytes, phase=0, lo_guard=GUARD_BYTES, hi_guard=GUARD_BYTES, key=0, device=None,
                 capacity=None):
        if not 0 <= phase <= 15:
            raise ValueError("phase must be 0..15")
        nbytes, lo_guard, hi_guard = int(nbytes), int(lo_guard), int(hi_guard)
        capacity = nbytes if capacity is None else int(capacity)
        if nbytes < 0 or capacity < nbytes or lo_guard < 1 or hi_guard < 1:
            raise ValueError("sizes")
        if device is None:
            device = torch.device("cuda:0")
        self.key, self.phase, self.capacity = key, phase, capacity
        total = lo_guard + capacity + hi_guard + 15
        self.buf = torch.empty(total, dtype=torch.uint8, device=device)
        # the lower guard absorbs the padding that puts the payload at `phase`; what is left of the 15 spare bytes
        # falls to the upper guard
        self.start = lo_guard + (phase - (self.buf.data_ptr() + lo_guard)) % 16
        self._stamp = torch.from_numpy(_stamp(key, total).copy()).to(device)
        self.reset(nbytes)
        assert self.ptr % 16 == phase

    def reset(self, nbytes=None):
        """Stamp the whole allocation again (payload included) and, if given, set a new payload size <= capacity."""
        if nbytes is not None:
            if not 0 <= int(nbytes) <= self.capacity:
                raise ValueError("nbytes beyond the capacity")
            self.nbytes = int(nbytes)
        self.buf.copy_(self._stamp)
        return self

    @property
    def ptr(self):
        """The payload's address."""
        return self.buf.data_ptr() + self.start

    @property
    def end(self):
        return self.start + self.nbytes

    def payload(self):
        """The payload as a uint8 view of the allocation."""
        return self.buf[self.start:self.end]

    def load(self, a):
        """Fill the payload with the bytes of a numpy array of exactly its size (padding bytes included)."""
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        if raw.size != self.nbytes:
            raise ValueError(f"{raw.size} bytes for a payload of {self.nbytes}")
        if raw.size:
            self.payload().copy_(torch.from_numpy(raw.copy()).to(self.buf.device))
        return self

    def read(self, npdt):
        """The payload on the host as a numpy array of `npdt`."""
        return self.payload().cpu().numpy().view(npdt)

    def snapshot(self):
        """A copy of the whole allocation, guards included, for unchanged_since()."""
        return self.buf.clone()

    def _regions(self, with_payload):
        r = [("lower", 0, self.start)]
        if with_payload:
            r.append(("payload", self.start, self.end))
        r.append(("upper", self.end, self.buf.numel()))
        return r

    def _compare(self, ref, with_payload, what):
        diffs = []
        for region, lo, hi in self._regions(with_payload):
            a, b = self.buf[lo:hi], ref[lo:hi]
            if hi == lo or torch.equal(a, b):
                continue
            idx = (a != b).nonzero()
            diffs.append(Diff(region, lo + int(idx[0]) - self.start, idx.shape[0]))
        return Check(diffs, what)

    def guards_intact(self):
        """Both guards still hold their stamp."""
        return self._compare(self._stamp, False, "guards")

    def unchanged_since(self, snapshot):
        """Guards and payload are byte-identical to `snapshot` (one comparison when nothing differs)."""
        if torch.equal(self.buf, snapshot):
            return Check([], "input")
        return self._compare(snapshot, True, "input")
