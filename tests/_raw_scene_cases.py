"""Shared pieces of the raw-scene tests (tests/test_raw_scene_host.py, tests/test_hip_raw_scene.py): the numpy definition of the group-feature
assembly, its inputs at the kernel's edges, and an in-process exchange that lets one process run every rank of a cut scene in turn."""
import numpy as np

SENTINEL = 7.25                       # exact in bfloat16: the columns outside a launch's window keep it bit for bit


def assemble_numpy(feats, cuts, nn, g0, out):
    """out[n, f, g0 + r] = feats[cuts[r] + nn[r, n], f]: roreg_group_feature_assemble in numpy (in place; nothing else is touched)."""
    for r in range(nn.shape[0]):
        out[:, :, g0 + r] = feats[cuts[r] + nn[r]]
    return out


def assemble_loops(feats, cuts, nn, g0, out):
    """The same, as the literal triple loop."""
    R, N = nn.shape
    for n in range(N):
        for f in range(feats.shape[1]):
            for r in range(R):
                out[n, f, g0 + r] = feats[cuts[r] + nn[r, n], f]
    return out


def kernel_case(seed, N, R, F):
    """-> (feats float32 [M,F], cuts int32 [R + 1], nn int64 [R,N]).  Every third item has one row; nn names every item's first row (keypoint 0) and
    last row (keypoint N - 1).  Half of feats' elements are exact ties of the bfloat16 rounding (low 16 bits 0x8000), with even and odd kept bits."""
    rng = np.random.default_rng([seed, N, R, F])
    rows = np.array([1 if r % 3 == 0 else int(rng.integers(2, 41)) for r in range(R)])
    cuts = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    nn = np.stack([rng.integers(0, rows[r], N) for r in range(R)]).astype(np.int64)
    nn[:, 0] = 0
    nn[:, -1] = rows - 1
    bits = rng.standard_normal((int(cuts[-1]), F)).astype(np.float32).view(np.uint32)
    tie = rng.random(bits.shape) < 0.5
    bits = np.where(tie, (bits & np.uint32(0xFFFF0000)) | np.uint32(0x8000), bits)
    kept = (bits[tie] >> 16) & 1
    assert kept.size == 0 or bits.size < 64 or (kept.min() == 0 and kept.max() == 1)
    return np.ascontiguousarray(bits).view(np.float32), cuts, nn


class Mailbox:
    """distributed.EqvExchange's interface for ranks that run one after the other in one process: a sender leaves its payloads in `box` (keyed
    by tag), a receiver that runs later copies them into its buffers.  Every transfer must go from a rank that runs earlier to one that runs later."""

    def __init__(self, rank, box):
        self.rank, self.box = rank, box
        self.landed = []
        self.bytes_sent = self.bytes_received = 0

    def start(self, transfers, get_eqv, alloc, tags=None):
        for tag, (s, i, src, dst) in zip(range(len(transfers)) if tags is None else tags, transfers):
            if src == self.rank:
                t = get_eqv(s, i)
                self.box[tag] = t.clone()
                self.bytes_sent += t.numel() * t.element_size()
            if dst == self.rank:
                buf = alloc(s, i)
                self.landed.append(((s, i), buf, tag))
                self.bytes_received += buf.numel() * buf.element_size()

    def wait(self):
        out = {}
        for key, buf, tag in self.landed:
            buf.copy_(self.box[tag])
            out[key] = buf
        self.landed = []
        return out


def rank_order(plan, scene):
    """The ranks that hold a range of `scene`, in the order of their first range: owners run before the ranks they ship to."""
    return sorted((r for r in range(len(plan)) if any(p[0] == scene for p in plan[r])), key=lambda r: min(p[1] for p in plan[r] if p[0] == scene))
