"""Launcher for the reference's own kernels (cudabits/arraylet2.cu + common.h, compiled for gfx950 by oracle/ref_kernels.py into
oracle/_ref/arraylet2.co): ctypes on the HIP runtime the process already holds -- hipModuleLoadData, hipModuleGetFunction,
hipModuleLaunchKernel -- with torch tensors as device memory, on torch's current stream.  Test plumbing; not a conftest.

The reference's kernels check no bounds (only updateLam has `i < colCount*sz`), so this launcher REFUSES, before any launch, every
shape they would index out of: see RefArraylet2.__init__ and _want.  Every buffer it hands out lies between two guard regions of a
fill pattern; check_guards() looks at all of them.  Launch shapes are the reference's (GPU/CUDA/Arraylet2.hs, cited per kernel)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from oracle import ref_kernels as recipe

CODE_OBJECT = recipe.CODE_OBJECT
GUARD_WORDS = 256                         # 1 KiB on each side of a buffer
GUARD_FILL = 0x7FC5A5A5                  # a quiet NaN as a float, an absurd index as an int
CLAMP = 2 * 18.714973875118524            # |message| when atanh_'s clamp fires (common.h:82-88, times -2 in selfProduct)


def available():
    return os.path.exists(CODE_OBJECT)


class HipError(RuntimeError):
    pass


_hip = None


def _runtime():
    """the libamdhip64 this process already runs on (torch's own copy when torch bundles one): a second runtime would see no GPU"""
    global _hip
    if _hip is None:
        import torch
        torch.cuda.init()
        path = None
        with open("/proc/self/maps") as maps:
            for line in maps:
                if "libamdhip64.so" in line:
                    path = line.split()[-1]
                    break
        if path is None:
            raise HipError("no libamdhip64.so is loaded in this process")
        L = C.CDLL(path)
        L.hipGetErrorString.restype = C.c_char_p
        L.hipGetErrorString.argtypes = [C.c_int]
        L.hipModuleLoadData.argtypes = [C.POINTER(C.c_void_p), C.c_char_p]
        L.hipModuleUnload.argtypes = [C.c_void_p]
        L.hipModuleGetFunction.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_char_p]
        L.hipModuleLaunchKernel.argtypes = [C.c_void_p] + [C.c_uint] * 7 + [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        _hip = L
    return _hip


def _check(rc, what):
    if rc != 0:
        raise HipError(f"{what}: HIP error {rc} ({_runtime().hipGetErrorString(rc).decode()})")


class Buf:
    """n 32-bit words of device memory between two guard regions; .t is the view a kernel gets (float32 or int32)"""

    def __init__(self, torch, dev, n, dtype, init=None):
        self.n, self.torch = int(n), torch
        self.raw = torch.full((self.n + 2 * GUARD_WORDS,), GUARD_FILL, dtype=torch.int32, device=dev)
        self.t = self.raw[GUARD_WORDS: GUARD_WORDS + self.n].view(dtype)
        if init is None:
            self.t.zero_()
        else:
            self.put(init)

    def put(self, a):
        a = np.ascontiguousarray(a).reshape(-1)
        assert a.shape == (self.n,), (a.shape, self.n)
        self.t.copy_(self.torch.from_numpy(a).to(self.t.dtype))

    def get(self):
        return self.t.cpu().numpy().copy()

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        raw = self.raw.cpu().numpy()
        return bool((raw[:GUARD_WORDS] == GUARD_FILL).all() and (raw[GUARD_WORDS + self.n:] == GUARD_FILL).all())


class RefArraylet2:
    """the reference's decoder state for one quasi-cyclic H: offsets [rowCount/sz][colCount] (-1: absent block), and launches of its
    kernels on buffers made by lam_buf() / mlet_buf() / done_buf()"""

    def __init__(self, sz, offsets, dev=0):
        offsets = np.ascontiguousarray(offsets, np.int32)
        if offsets.ndim != 2:
            raise ValueError("offsets must be [block rows][block columns]")
        self.sz, self.colCount = int(sz), int(offsets.shape[1])
        self.rowCount = int(offsets.shape[0]) * self.sz
        # selfProduct's grid is rowCount/4 workgroups of (4, colCount) threads (Arraylet2.hs:213-216); tanhTransform's is rowCount/32
        # workgroups of 32 rows: a remainder would leave rows undone, a larger workgroup does not launch
        if self.sz < 1 or self.colCount < 1 or self.rowCount % 4 or 4 * self.colCount > 1024:
            raise ValueError(f"refused: rowCount {self.rowCount} must be a multiple of 4 and 4 * colCount ({self.colCount}) at most 1024")
        # lamIndex (common.h:90-98) and updateLam (:163-164) index lam and newMLet by (off + j) % sz and (i + sz - off) % sz
        if offsets.min() < -1 or offsets.max() >= self.sz:
            raise ValueError(f"refused: an offset outside [-1, {self.sz})")
        if not available():
            raise FileNotFoundError(CODE_OBJECT)
        import torch
        self.torch, self.dev = torch, torch.device("cuda", dev)
        self.offsets_host = offsets
        self.bufs = []
        self.offsets = self._buf(offsets.size, torch.int32, offsets)
        self._hip = _runtime()
        self._image = open(CODE_OBJECT, "rb").read()
        self._module = C.c_void_p()
        _check(self._hip.hipModuleLoadData(C.byref(self._module), self._image), "hipModuleLoadData")
        self._fn = {}

    def close(self):
        if self._module:
            self.torch.cuda.synchronize()
            _check(self._hip.hipModuleUnload(self._module), "hipModuleUnload")
            self._module = C.c_void_p()

    # ---- buffers -----------------------------------------------------------------------------------------------------------------
    def _buf(self, n, dtype, init=None):
        b = Buf(self.torch, self.dev, n, dtype, init)
        self.bufs.append(b)
        return b

    def lam_buf(self, init=None):
        return self._buf(self.colCount * self.sz, self.torch.float32, init)

    def mlet_buf(self, init=None):
        """[rowCount][colCount] floats, ZERO-filled unless init is given.  (The reference leaves newMLet as mallocArray returned it,
        Arraylet2.hs:123, and updateLam adds its absent-block slots: it assumes fresh device memory is zero.)"""
        return self._buf(self.rowCount * self.colCount, self.torch.float32, init)

    def done_buf(self, value=0):
        return self._buf(1, self.torch.int32, np.array([value], np.int32))

    def check_guards(self):
        self.torch.cuda.synchronize()
        bad = [k for k, b in enumerate(self.bufs) if not b.guards_intact()]
        assert not bad, f"a kernel wrote outside buffers {bad}"

    # ---- launches ----------------------------------------------------------------------------------------------------------------
    def _want(self, buf, n, dtype, name):
        if not isinstance(buf, Buf) or buf not in self.bufs or buf.n != n or buf.t.dtype != dtype:
            raise ValueError(f"refused: {name} must be a buffer of this launcher with exactly {n} {dtype} words")

    def _launch(self, name, grid, block, shared, args):
        if name not in self._fn:
            f = C.c_void_p()
            _check(self._hip.hipModuleGetFunction(C.byref(f), self._module, name.encode()), f"hipModuleGetFunction({name})")
            self._fn[name] = f
        threads = block[0] * block[1] * block[2]
        assert 0 < threads <= 1024 and min(grid) >= 1 and shared <= 64 * 1024
        vals = [C.c_void_p(a.ptr) if isinstance(a, Buf) else C.c_int(a) for a in args]
        params = (C.c_void_p * len(vals))(*[C.cast(C.byref(v), C.c_void_p) for v in vals])
        stream = C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)
        _check(self._hip.hipModuleLaunchKernel(self._fn[name], grid[0], grid[1], grid[2], block[0], block[1], block[2], shared, stream, params, None),
               f"hipModuleLaunchKernel({name})")

    def _dims(self):
        return [self.rowCount, self.colCount, self.sz, self.offsets]

    def selfProduct(self, lam, mLet, newMLet):
        """Arraylet2.hs:213-226: grid (rowCount/4), block (4, colCount), 4 * colCount floats of LDS"""
        f32 = self.torch.float32
        self._want(lam, self.colCount * self.sz, f32, "lam")
        self._want(mLet, self.rowCount * self.colCount, f32, "mLet")
        self._want(newMLet, self.rowCount * self.colCount, f32, "newMLet")
        if mLet is newMLet:
            raise ValueError("refused: mLet and newMLet are two arrays")
        self._launch("selfProduct", (self.rowCount // 4, 1, 1), (4, self.colCount, 1), 4 * self.colCount * 4, [lam, mLet, newMLet] + self._dims())

    def updateLam(self, lam, newMLet):
        """Arraylet2.hs:248-262: grid (sz), block (colCount)"""
        self._want(lam, self.colCount * self.sz, self.torch.float32, "lam")
        self._want(newMLet, self.rowCount * self.colCount, self.torch.float32, "newMLet")
        self._launch("updateLam", (self.sz, 1, 1), (self.colCount, 1, 1), 0, [lam, newMLet] + self._dims())

    def parityRowResults(self, done, lam):
        """Arraylet2.hs:176-190: grid (1, rowCount), block (colCount).  Its barrier stands under `if (!*done)`, a racy read of global
        memory (common.h:222-225): only with ONE wave per workgroup is that read wave-uniform and the barrier trivially met."""
        if self.colCount > 64:
            raise ValueError(f"refused: parityRowResults with colCount {self.colCount} > 64 has a barrier under a condition that waves of one workgroup can disagree on")
        self._want(done, 1, self.torch.int32, "done")
        self._want(lam, self.colCount * self.sz, self.torch.float32, "lam")
        self._launch("parityRowResults", (1, self.rowCount, 1), (self.colCount, 1, 1), 0, [done, lam] + self._dims())

    def tanhTransform(self, mLet, lam):
        """the commented-out launch at Arraylet2.hs:200-211, with 32 rows per workgroup: grid (colCount, rowCount/32), block (1, 32)"""
        if self.rowCount % 32:
            raise ValueError(f"refused: tanhTransform with rowCount {self.rowCount} not a multiple of 32")
        self._want(mLet, self.rowCount * self.colCount, self.torch.float32, "mLet")
        self._want(lam, self.colCount * self.sz, self.torch.float32, "lam")
        self._launch("tanhTransform", (self.colCount, self.rowCount // 32, 1), (1, 32, 1), 0, [mLet, lam] + self._dims())


def edge_slots(graph, sz, offsets):
    """slot j * colCount + i of the arraylet matrix for every edge of graph (CSR order: row j, ascending column n; i = n // sz).
    Derived from the graph alone; that every edge falls on a present block, one edge per slot, is asserted."""
    colCount = offsets.shape[1]
    rows = np.repeat(np.arange(graph.M), np.diff(graph.row_ptr))
    slots = rows * colCount + graph.col_idx // sz
    assert len(np.unique(slots)) == graph.E and (offsets[rows // sz, graph.col_idx // sz] >= 0).all()
    assert graph.E == int((offsets >= 0).sum()) * sz
    return slots.astype(np.int64)
