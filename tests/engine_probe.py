"""What the stage-by-stage tests of the three decode engines share (tests/test_gpu_{gpt,rar,cham}_kernels.py): one live engine
behind its wmar_<engine>_probe_run / _probe_copy / _probe_plan entries, the parser of the plan text, the figure printer and the
module's engine cache.  A test file subclasses EngineProbe and states only what is its own: shapes, weights, element types, its
stages and what its plan must say; a fourth engine's tests start here.  (No conftest.py: the fixtures stay in the test files.)"""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch


def say(prefix, width):
    """the printer of a file's figure lines: `PREFIX tag  k=v k=v ...` (floats to three digits)"""
    fmt = "%s %%-%ds %%s" % (prefix, width)
    return lambda tag, **figs: print(fmt % (tag, " ".join("%s=%s" % (k, ("%.3g" % v) if isinstance(v, float) else v) for k, v in figs.items())))


@contextlib.contextmanager
def engine_env(names):
    """the creation-time switches of an engine: each name is "1" inside; afterwards it has its previous value, or is unset again"""
    old = {e: os.environ.get(e) for e in names}
    for e in names:
        os.environ[e] = "1"
    try:
        yield
    finally:
        for e, v in old.items():
            if v is None:
                del os.environ[e]
            else:
                os.environ[e] = v


def parse_plan(text, list_keys=("stages",), ints=True):
    """`k=v k=v ... [kernels=...]` as a dict.  Values that are integer literals become ints (unless ints=False), values of list_keys
    lists; behind " kernels=" the raw string is `kernels`, and `roles` its `role=kernel;role=kernel` pairs where every item is one."""
    head, sep, kernels = text.partition(" kernels=")
    out = {}
    for item in head.split():
        k, v = item.split("=", 1)
        out[k] = v.split(",") if k in list_keys else int(v) if ints and re.fullmatch(r"-?\d+", v) else v
    if sep:
        out["kernels"] = kernels
        items = kernels.split(";")
        if all("=" in it for it in items):
            out["roles"] = dict(it.split("=", 1) for it in items)
    return out


class EngineCache:
    """a test module's engines, created on first use and closed when the module ends"""

    def __init__(self):
        self.engines = {}

    def get(self, key, make):
        if key not in self.engines:
            self.engines[key] = make()
        return self.engines[key]

    def close_all(self):
        for pr in self.engines.values():
            pr.close()
        self.engines.clear()


def dev(a, dtype=torch.int64):
    """a host array (or None) on the device"""
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype).cuda()


def _signed(a):
    """numpy has the unsigned views the kernels' bit patterns are compared in, torch the signed types of the same width"""
    a = np.ascontiguousarray(a)
    return a.view(np.int16) if a.dtype == np.uint16 else a.view(np.int64) if a.dtype == np.uint64 else a


class EngineProbe:
    """One engine and stage access to it."""
    ENGINE = None           # "gpt" | "rar" | "cham"
    DTYPES = {}             # buffer name -> torch dtype (float32 where absent)
    U64 = frozenset()       # int64 buffers that get() hands out as uint64

    def _create(self, config, state, env=(), dtype=torch.float32):
        from wmar_amd import _lib
        self._lib, self.L = _lib, _lib.load()
        self._copy, self._run, self._plan, self._destroy = (getattr(self.L, "wmar_%s_%s" % (self.ENGINE, f))
                                                            for f in ("probe_copy", "probe_run", "probe_plan", "destroy"))
        tensors = {k: torch.as_tensor(v).to("cuda", dtype).contiguous() for k, v in state.items()}
        names, ptrs, n = _lib.tensor_table(tensors)
        h = C.c_void_p()
        with engine_env(env):
            _lib.check(getattr(self.L, "wmar_%s_create" % self.ENGINE)(C.byref(config), names, ptrs, n, _lib.stream_ptr(), C.byref(h)))
        torch.cuda.synchronize()
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self._destroy(self.h)
            self.h = None

    __del__ = close

    # ---- raw buffers
    def _dt(self, name):
        return self.DTYPES.get(name, torch.float32)

    def _copy_checked(self, name, layer, ptr, nbytes, to_engine):
        n = self._copy(self.h, name.encode(), layer, ptr, nbytes, to_engine, self._lib.stream_ptr())
        if n < 0:
            self._lib.check(int(n))
        return int(n)

    def size(self, name, layer=0):
        return self._copy_checked(name, layer, None, 0, 0)

    def has(self, name):
        return self._copy(self.h, name.encode(), 0, None, 0, 0, self._lib.stream_ptr()) > 0

    def get_dev(self, name, layer=0):
        n, dt = self.size(name, layer), self._dt(name)
        t = torch.empty(n // dt.itemsize, dtype=dt, device="cuda")
        self._copy_checked(name, layer, t.data_ptr(), n, 0)
        return t

    def get(self, name, layer=0):
        a = self.get_dev(name, layer).cpu().numpy()
        return a.view(np.uint16) if a.dtype == np.int16 else (a.view(np.uint64) if name in self.U64 else a)

    def put(self, name, a, layer=0):
        if isinstance(a, np.ndarray):
            a = torch.from_numpy(_signed(a))
        t = a.to("cuda").contiguous().view(-1)
        assert t.dtype == self._dt(name), (name, t.dtype)
        assert t.numel() * t.element_size() == self.size(name, layer), (name, t.numel())
        self._copy_checked(name, layer, t.data_ptr(), t.numel() * t.element_size(), 1)

    def fill(self, name, value, layer=0):
        dt = self._dt(name)
        self.put(name, torch.full((self.size(name, layer) // dt.itemsize,), value, dtype=dt, device="cuda"), layer)

    def put_front(self, name, flat, layer=0, rest=None):
        """flat into the front of a buffer; the rest keeps its contents, or is set to `rest`"""
        t = self.get_dev(name, layer)
        if rest is not None:
            t.fill_(rest)
        src = torch.from_numpy(_signed(flat)).cuda().view(-1)
        t[:src.numel()] = src
        self.put(name, t, layer)

    # ---- stages
    def _checked(self, rc):
        """a launch that fails on the device ends the session: nothing more is started on a GPU that has faulted"""
        try:
            self._lib.check(rc)
        except self._lib.WmarError as e:
            pytest.exit("stopping: %s" % e, returncode=3)

    def _call(self, fn, rows, vocab, *args, want_logits=True):
        """fn(engine, *args, logits_dev, stream), a probe run or a whole-step entry, under _checked; device tensors among args go in as
        pointers; returns the [rows, vocab] logits if wanted"""
        lg = torch.empty(rows, vocab, dtype=torch.float32, device="cuda") if want_logits else None
        self._checked(fn(self.h, *(a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args), lg.data_ptr() if want_logits else None,
                         self._lib.stream_ptr()))
        if want_logits:
            torch.cuda.synchronize()
            return lg.cpu().numpy()

    def plan_text(self, *args, buflen=4096):
        buf = C.create_string_buffer(buflen)
        self._lib.check(self._plan(self.h, *args, buf, buflen))
        return buf.value.decode()
