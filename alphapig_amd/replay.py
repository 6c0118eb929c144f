"""Replay buffers of position CODES: what the self-play exchange delivers (240-byte code rows, pi, z -- 1 144 B per ply on
15x15) stored as it arrives, un-augmented, and the mini-batch decoded and rotated when it is drawn -- the opt-in
alternative (`replay` = "compact" / "device" in TrainPipeline's configuration) to pipeline.ReplayBuffer, the reference's
deque of 8x augmented float32 tuples (train_mxnet.py:59, :115-135; 9 000 B of array data per entry).

  RingIndex            the arithmetic both backends share: which (tuple, symmetry) logical entry i of the reference's
                       deque is, and which ring slot holds that tuple
  CompactReplayBuffer  storage and gather on the host (NumPy); needs no GPU, and states what the kernel must produce
  DeviceReplayBuffer   storage in device memory, gather by replay_gather_kernel (csrc/replay.h): nothing of a mini-batch
                       goes through the host except its k entry words
  planes_to_codes      the inverse of TreePool.codes_to_planes, for sources that yield planes (the SGF bootstrap)

Both buffers draw `rng.sample(range(len), k)` -- the same draws from the same generator state as ReplayBuffer.sample --
and return train.DeviceBatch(states [k][c_in][H][W], pis [k][HW], zs [k]) with the bits the tuple path stacks.
"""
import ctypes as C

import numpy as np

from . import _native
from .augment import dihedral_tables
from .train import DeviceBatch
from .treepool import TreePool


class RingIndex(object):
    """The reference's `deque(maxlen=M)` holds AUGMENTED entries, 8 per tuple in get_equi_data's order, and M need not be a
    multiple of 8.  With A entries appended so far the deque holds n = min(A, M); logical entry i (0 = oldest) is absolute
    entry a = A - n + i = symmetry a % 8 of tuple a // 8.  The live entries touch at most ceil(M / 8) + 1 tuples, so a ring
    of that many tuple slots (slot = tuple number mod capacity) holds them all."""

    def __init__(self, maxlen):
        self.maxlen = int(maxlen)
        if self.maxlen < 1:
            raise ValueError("maxlen must be positive")
        self.capacity = (self.maxlen + 7) // 8 + 1
        self.appended = 0                   # A: augmented entries appended so far (8 per tuple)

    def __len__(self):
        return min(self.appended, self.maxlen)

    def extend(self, n_tuples):
        """Append n_tuples tuples -> (skip, [(slot, count), ...]): the first `skip` of them are dead on arrival (more tuples
        than slots), the others go to the ring in order, `count` tuples from `slot` on per segment (two at the wrap)."""
        n_tuples = int(n_tuples)
        skip = max(0, n_tuples - self.capacity)
        first = self.appended // 8 + skip
        self.appended += 8 * n_tuples
        segs, left = [], n_tuples - skip
        while left:
            slot = first % self.capacity
            cnt = min(left, self.capacity - slot)
            segs.append((slot, cnt))
            first += cnt
            left -= cnt
        return skip, segs

    def locate(self, i):
        """logical entry i -> (tuple number, symmetry)"""
        n = len(self)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError(i)
        a = self.appended - n + i
        return a // 8, a % 8

    def word(self, i):
        """logical entry i -> its entry word slot * 8 + symmetry"""
        t, k = self.locate(i)
        return (t % self.capacity) * 8 + k

    def sample(self, rng, k):
        """`rng.sample(range(len), k)` -> int32 [k] entry words"""
        return np.array([self.word(i) for i in rng.sample(range(len(self)), k)], dtype=np.int32).reshape(-1)


def planes_to_codes(states):
    """states [n][9 or 4][H][W] (Board.current_state's planes, top row first) -> codes u8 [n][code stride], the rows
    TreePool.codes_to_planes turns back into exactly these planes.  9 planes: own / opponent stones are planes 6 / 7, a
    stone's age is the number of set planes among (6, 4, 2, 0) resp. (7, 5, 3, 1) minus one, plane 8 is the colour.
    4 planes: planes 0 / 1, plane 2 marks the last move (age 0; every other stone gets age 1), plane 3 the colour."""
    st = np.asarray(states)
    if st.ndim != 4 or st.shape[1] not in (9, 4):
        raise ValueError("states must be [n][9 or 4][H][W]")
    n, c, h, w = st.shape
    on = st != 0
    if c == 9:
        own, opp = on[:, 6], on[:, 7]
        age_own = on[:, 6].astype(np.uint8) + on[:, 4] + on[:, 2] + on[:, 0]
        age_opp = on[:, 7].astype(np.uint8) + on[:, 5] + on[:, 3] + on[:, 1]
        grid = np.where(own, age_own, 0) + np.where(opp & ~own, 4 + age_opp, 0)       # 1 + age / 5 + age
    else:
        own, opp = on[:, 0], on[:, 1]
        age1 = 2 - on[:, 2].astype(np.uint8)                                         # 1 + age
        grid = np.where(own, age1, 0) + np.where(opp & ~own, 4 + age1, 0)
    codes = np.zeros((n, (h * w + 1 + 15) // 16 * 16), dtype=np.uint8)
    codes[:, :h * w] = grid[:, ::-1].reshape(n, h * w)            # codes are bottom-row-first
    codes[:, h * w] = on[:, c - 1, 0, 0]
    return codes


class _Decoder(object):
    """What TreePool.codes_to_planes reads of its pool: the host library and the board -- no game slots, no trees"""

    def __init__(self, height, width):
        self.L = _native.host()
        self.height, self.width = int(height), int(width)
        self.code_stride = self.L.apzh_code_stride(self.height, self.width)

    def _ck(self, rc):
        if rc < 0:
            raise RuntimeError("%s (code %d)" % (self.L.apzh_last_error().decode(), rc))
        return rc

    def codes_to_planes(self, codes, n_planes):
        return TreePool.codes_to_planes(self, codes, n_planes)


class _CodeBuffer(object):
    """The interface of both backends; the storage itself (`_alloc`, `_write`, `_read`, `_rows`, `_gather`) is the backend's."""

    def __init__(self, maxlen, height, width, c_in=9):
        if int(height) != int(width):
            raise ValueError("the code replay buffers rotate boards: they need a square board, not %dx%d" % (height, width))
        if c_in not in (9, 4):
            raise ValueError("c_in must be 9 or 4")
        self.ring = RingIndex(maxlen)
        self.maxlen = self.ring.maxlen
        self.height, self.width, self.c_in = int(height), int(width), int(c_in)
        self.hw = self.height * self.width
        self._dec = _Decoder(height, width)
        self.code_stride = self._dec.code_stride
        self._alloc(self.ring.capacity)

    def __len__(self):
        return len(self.ring)

    def extend_codes(self, codes, pis, zs):
        """codes u8 [t][code stride], pis [t][HW], zs [t]: t tuples as the self-play exchange delivers them"""
        codes = np.ascontiguousarray(codes, dtype=np.uint8).reshape(-1, self.code_stride)
        pis = np.ascontiguousarray(pis, dtype=np.float32).reshape(-1, self.hw)
        zs = np.ascontiguousarray(zs, dtype=np.float32).reshape(-1)
        t = len(codes)
        if len(pis) != t or len(zs) != t:
            raise ValueError("codes, pis and zs must hold the same number of tuples")
        at, segs = self.ring.extend(t)
        for slot, cnt in segs:
            self._write(slot, codes[at:at + cnt], pis[at:at + cnt], zs[at:at + cnt])
            at += cnt

    def extend_planes(self, states, pis, zs):
        """The same for tuples that come as planes (the SGF bootstrap): stored as the codes that reproduce them"""
        states = np.asarray(states, dtype=np.float32).reshape(-1, self.c_in, self.height, self.width)
        codes = planes_to_codes(states)
        if not np.array_equal(self._dec.codes_to_planes(codes, self.c_in), states):
            raise ValueError("extend_planes: these planes are not the planes of a position (no code row reproduces them)")
        self.extend_codes(codes, pis, zs)

    # ---- checkpoint: the live tuples only, oldest first
    def _live(self):
        """-> (number of the oldest live tuple, how many are live, their ring segments [(slot, count)] -- two at the wrap)"""
        A, n, cap = self.ring.appended, len(self.ring), self.ring.capacity
        if A == 0:
            return 0, 0, []
        first = (A - n) // 8
        count = (A + 7) // 8 - first
        slot = first % cap
        head = min(count, cap - slot)
        return first, count, [(slot, head)] + ([(0, count - head)] if count > head else [])

    def state(self):
        """{"meta": maxlen, board, c_in and the count of entries appended so far; "codes" / "pi" / "z": the tuples the live
        entries belong to -- tuple numbers (appended - len) // 8 to ceil(appended / 8) - 1 -- in order} as host arrays."""
        _, count, segs = self._live()
        parts = [self._read(slot, cnt) for slot, cnt in segs]
        cat = lambda j, empty: np.concatenate([p[j] for p in parts]) if parts else empty
        return {"meta": {"maxlen": self.maxlen, "height": self.height, "width": self.width, "c_in": self.c_in,
                         "appended": int(self.ring.appended)},
                "codes": cat(0, np.zeros((0, self.code_stride), np.uint8)), "pi": cat(1, np.zeros((0, self.hw), np.float32)),
                "z": cat(2, np.zeros(0, np.float32))}

    def load_state(self, state):
        """The inverse of state(), into a buffer of the same maxlen, board and c_in (anything else: ValueError)."""
        meta = state["meta"]
        for k in ("maxlen", "height", "width", "c_in"):
            if int(meta[k]) != getattr(self, k):
                raise ValueError("this replay state was taken with %s=%r, the buffer has %s=%r" % (k, meta[k], k, getattr(self, k)))
        appended = int(meta["appended"])
        codes = np.ascontiguousarray(state["codes"], dtype=np.uint8).reshape(-1, self.code_stride)
        pis = np.ascontiguousarray(state["pi"], dtype=np.float32).reshape(-1, self.hw)
        zs = np.ascontiguousarray(state["z"], dtype=np.float32).reshape(-1)
        old = self.ring.appended
        self.ring.appended = appended
        _, count, segs = self._live()
        if appended < 0 or appended % 8 or not len(codes) == len(pis) == len(zs) == count:
            self.ring.appended = old
            raise ValueError("this replay state holds %d tuples; %d appended entries keep %d alive" % (len(codes), appended, count))
        at = 0
        for slot, cnt in segs:
            self._write(slot, codes[at:at + cnt], pis[at:at + cnt], zs[at:at + cnt])
            at += cnt

    def sample(self, rng, k):
        """-> DeviceBatch(states, pis, zs) of k entries, drawn like ReplayBuffer.sample draws them"""
        return self._gather(self.ring.sample(rng, k))

    def entry(self, i):
        """Logical entry i as one host (state [c_in][H][W], pi [HW], z) tuple: what the reference's deque holds at i"""
        t, k = self.ring.locate(i)
        codes, pi, z = self._rows(t % self.ring.capacity)
        ps, pp = dihedral_tables(self.height)
        planes = self._dec.codes_to_planes(codes, self.c_in)[0]
        return planes.reshape(self.c_in, -1)[:, ps[k]].reshape(planes.shape), pi[pp[k]], z


class CompactReplayBuffer(_CodeBuffer):
    """Host storage: codes u8 [cap][code stride], pi f32 [cap][HW], z f32 [cap] -- an eighth of the tuples and 1 144 B
    instead of 9 000 B for each of them -- and a NumPy gather that decodes and rotates only the rows a mini-batch draws."""

    def _alloc(self, cap):
        self.codes = np.zeros((cap, self.code_stride), dtype=np.uint8)
        self.pi = np.zeros((cap, self.hw), dtype=np.float32)
        self.z = np.zeros(cap, dtype=np.float32)

    def _write(self, slot, codes, pis, zs):
        self.codes[slot:slot + len(codes)] = codes
        self.pi[slot:slot + len(codes)] = pis
        self.z[slot:slot + len(codes)] = zs

    def _rows(self, slot):
        return self.codes[slot:slot + 1], self.pi[slot], self.z[slot]

    def _read(self, slot, cnt):
        return self.codes[slot:slot + cnt].copy(), self.pi[slot:slot + cnt].copy(), self.z[slot:slot + cnt].copy()

    def _gather(self, words):
        slots, syms = words >> 3, words & 7
        ps, pp = dihedral_tables(self.height)
        k = len(words)
        planes = self._dec.codes_to_planes(self.codes[slots], self.c_in).reshape(k, self.c_in, self.hw)
        states = np.take_along_axis(planes, ps[syms][:, None, :], axis=2).reshape(k, self.c_in, self.height, self.width)
        return DeviceBatch(states, np.take_along_axis(self.pi[slots], pp[syms], axis=1), self.z[slots])


class DeviceReplayBuffer(_CodeBuffer):
    """The same three arrays as torch tensors on the trainer's device.  extend_codes copies the new rows into the ring on
    torch's current stream; sample uploads the k entry words and launches replay_gather_kernel on the same stream -> a
    DeviceBatch of device tensors, what HipTrainer.upload returns.  Belongs to ONE thread (the trainer's), like the list."""

    def __init__(self, maxlen, height, width, c_in=9, device=0):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceReplayBuffer needs a GPU (replay='compact' keeps the codes on the host)")
        _native.hip()                          # raises when libalphapig_hip.so is missing
        self.torch = torch
        self.device = torch.device("cuda", int(device))
        _CodeBuffer.__init__(self, maxlen, height, width, c_in)

    def _alloc(self, cap):
        torch = self.torch
        self.codes = torch.zeros((cap, self.code_stride), dtype=torch.uint8, device=self.device)
        self.pi = torch.zeros((cap, self.hw), dtype=torch.float32, device=self.device)
        self.z = torch.zeros((cap,), dtype=torch.float32, device=self.device)
        torch.cuda.synchronize(self.device)    # whichever stream the owner works on later finds the ring zeroed

    def nbytes(self):
        """The ring's footprint in device memory"""
        return sum(int(t.numel()) * t.element_size() for t in (self.codes, self.pi, self.z))

    def _write(self, slot, codes, pis, zs):
        torch = self.torch
        n = len(codes)
        self.codes[slot:slot + n].copy_(torch.from_numpy(codes))
        self.pi[slot:slot + n].copy_(torch.from_numpy(pis))
        self.z[slot:slot + n].copy_(torch.from_numpy(zs))

    def _rows(self, slot):
        return self.codes[slot:slot + 1].cpu().numpy(), self.pi[slot].cpu().numpy(), self.z[slot].cpu().numpy()[()]

    def _read(self, slot, cnt):
        return tuple(t[slot:slot + cnt].cpu().numpy() for t in (self.codes, self.pi, self.z))

    def _gather(self, words):
        from . import hipconv
        return DeviceBatch(*hipconv.replay_gather(self.codes, self.pi, self.z, words, self.height, self.width, self.c_in))
