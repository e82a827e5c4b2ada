"""RowArena -- reserved, double-buffered row storage for the per-Gaussian state (the six raw parameters, their Adam
moments, `send_to_gpui_cnt` and the four zeroed statistics), so that a densification event
(densification_ops.densify_and_prune_fused) moves rows from one half to the other instead of building every tensor
anew with `torch.cat` / boolean indexing (scene/gaussian_model.py:789-921 of the reference).

Every tensor has two HALVES of `capacity` rows; the live tensor is the view `half[:n]` of one of them.  An event reads
the live half (or, the first time, the tensor the model was built with) and writes the other one; the next event goes
the other way.  Nothing is allocated while the row count stays inside the capacity.

Memory trade: the arena keeps 2 x capacity rows of every tensor for the whole run (708 B of parameters and moments per
row and half).  The `cat` path reaches the same peak, old and new tensor side by side, only for the duration of an event
and gives it back to the caching allocator afterwards; the arena keeps it, and in exchange an event costs no allocator
traffic and no allocation can fail in the middle of a run.

Lifetime rule: a view handed out by an event stays valid until the event AFTER the next one starts writing its half,
i.e. views of the half that an event READ are dead once the next event begins.  Code that keeps a tensor across
events (a captured graph, a pending deferred backward, a checkpoint in flight) must `clone()` it or be reset before the
event -- as it must already with the allocating path, where the old tensors are freed.

Pure torch, any device: the host logic is tested on CPU tensors."""
import torch


def _headroom(rows):
    """1.1 x rows, rounded up (integers: 1.1 * 100 is 110.00000000000001 in floating point)"""
    return (11 * int(rows) + 9) // 10


def _grown(capacity):
    """1.5 x capacity, rounded up: a row count beyond the capacity grows it to max(this, 1.1 x rows)"""
    return (3 * int(capacity) + 1) // 2


class RowArena:
    def __init__(self, rows, device, capacity=None):
        self.device = torch.device(device)
        self.capacity = max(int(capacity) if capacity is not None else _headroom(rows), 1)
        self._halves = {}    # key -> [tensor | None, tensor | None], each [capacity_at_allocation, ...]
        self._stats = {}     # name -> tensor [capacity_at_allocation, ...]
        self._scratch = {}   # name -> flat tensor
        self.events = 0
        self.growths = 0

    def reserve(self, rows):
        """make room for `rows` rows; True when the capacity had to grow (the halves written from now on are allocated at
        the new capacity, the old ones are released when their last view goes)"""
        if rows <= self.capacity:
            return False
        self.capacity = max(_grown(self.capacity), _headroom(rows))
        self.growths += 1
        return True

    @staticmethod
    def _same_storage(a, b):
        return a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()

    def half_of(self, key, t):
        """index of the half of `key` that tensor `t` is a view of, or None"""
        for i, h in enumerate(self._halves.get(key, (None, None))):
            if h is not None and t.device == h.device and self._same_storage(t, h):
                return i
        return None

    def destination(self, key, src, rows):
        """the half of `key` that `src` does NOT live in, with room for `rows` rows: a [capacity, *src.shape[1:]] tensor
        of src's dtype (allocated on first use and after a growth; its contents are undefined)"""
        self.reserve(rows)
        halves = self._halves.setdefault(key, [None, None])
        cur = self.half_of(key, src)
        i = 0 if cur != 0 else 1
        h = halves[i]
        if h is None or h.shape[0] < rows or h.shape[1:] != src.shape[1:] or h.dtype != src.dtype:
            h = halves[i] = torch.empty((self.capacity,) + tuple(src.shape[1:]), dtype=src.dtype, device=self.device)
        return h

    def extend(self, key, t, rows):
        """the first `rows` rows of the half that `t` lives in, `t` being its first t.shape[0] rows: the longer view of the
        SAME storage, nothing moves (the rows beyond t are undefined until the caller writes them).  A tensor that does
        not live in the arena yet -- or whose half is too short, after a growth -- is copied once into a reserved half.
        For in-place row growth (mcmc.MCMCStrategy.relocate_and_grow)."""
        self.reserve(rows)
        halves = self._halves.setdefault(key, [None, None])
        cur = self.half_of(key, t)
        if cur is not None and halves[cur].shape[0] >= rows and t.data_ptr() == halves[cur].data_ptr():
            return halves[cur][:rows]
        h = torch.empty((self.capacity,) + tuple(t.shape[1:]), dtype=t.dtype, device=self.device)
        h[:t.shape[0]].copy_(t)
        halves[cur if cur is not None else 0] = h  # (a half that was too short goes when its last view does)
        return h[:rows]

    def release_other(self, key, live):
        """drop the half of `key` that `live` is not a view of when it is smaller than the capacity (after a growth: the
        next event would have to replace it anyway, so its memory goes back now rather than then)"""
        halves = self._halves.get(key)
        if halves is None:
            return
        cur = self.half_of(key, live)
        for i, h in enumerate(halves):
            if i != cur and h is not None and h.shape[0] < self.capacity:
                halves[i] = None

    def zeros(self, name, rows, tail=(), dtype=torch.float32):
        """a zero-filled [rows, *tail] view of the reserved statistics buffer `name`"""
        self.reserve(rows)
        buf = self._stats.get(name)
        if buf is None or buf.shape[0] < rows or tuple(buf.shape[1:]) != tuple(tail) or buf.dtype != dtype:
            buf = self._stats[name] = torch.empty((self.capacity,) + tuple(tail), dtype=dtype, device=self.device)
        return buf[:rows].zero_()

    def scratch(self, name, numel, dtype):
        """a reserved flat work buffer of at least `numel` elements (the plan's ranks and workspace)"""
        buf = self._scratch.get(name)
        if buf is None or buf.numel() < numel or buf.dtype != dtype:
            buf = self._scratch[name] = torch.empty(max(int(numel), 1), dtype=dtype, device=self.device)
        return buf

    def nbytes(self):
        ts = [h for hs in self._halves.values() for h in hs if h is not None]
        ts += list(self._stats.values()) + list(self._scratch.values())
        return sum(t.numel() * t.element_size() for t in ts)
