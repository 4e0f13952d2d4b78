"""CPU: the backward probes and the training entries of the C ABI are declared, listed and exported, and refuse null arguments
without a GPU."""
import ctypes as C
import os
import re

from tests.conftest import REPO

ENTRIES = ["wmar_vq_train_create", "wmar_vq_train_destroy", "wmar_vq_train_device_bytes", "wmar_vq_train_set_weights", "wmar_vq_train_encode",
           "wmar_vq_train_encode_backward", "wmar_vq_train_decode", "wmar_vq_train_decode_backward", "wmar_vq_train_get_grads",
           "wmar_vq_probe_conv_backward", "wmar_vq_probe_gn_backward", "wmar_vq_probe_attn_backward"]


def test_new_symbols_are_declared_listed_and_exported():
    from wmar_amd import _lib
    L = _lib.load()
    header = open(os.path.join(REPO, "include", "wmar_hip.h")).read()
    declared = set(re.findall(r"\b(wmar_[a-z0-9_]+)\s*\(", header))
    for s in ENTRIES:
        assert s in declared and s in _lib.SYMBOLS and hasattr(L, s), s


def test_null_arguments_are_refused_with_a_message():
    from wmar_amd import _lib
    L = _lib.load()
    buf = C.create_string_buffer(64)
    calls = [lambda: L.wmar_vq_train_create(None, None, None, 0, None, None),
             lambda: L.wmar_vq_train_set_weights(None, None, None, 0, None),
             lambda: L.wmar_vq_train_encode(None, None, 1, None, None),
             lambda: L.wmar_vq_train_encode_backward(None, None, 1, None, None),
             lambda: L.wmar_vq_train_decode(None, None, 1, None, None),
             lambda: L.wmar_vq_train_decode_backward(None, None, 1, None, None),
             lambda: L.wmar_vq_train_get_grads(None, None, None, 0, 0, None),
             lambda: L.wmar_vq_probe_conv_backward(None, 1, 1, 1, None, None, 1, 8, 8, 1, 0, None, None, None, buf, 64, None),
             lambda: L.wmar_vq_probe_gn_backward(None, None, None, None, None, 1, 64, 32, 0, None, None, None, buf, 64, None),
             lambda: L.wmar_vq_probe_attn_backward(None, None, None, None, 1, 8, 8, 64, None, None, None, buf, 64, None)]
    for call in calls:
        assert call() == -1                                   # WMAR_EINVAL
        assert b"null argument" in L.wmar_last_error()
    assert L.wmar_vq_train_device_bytes(None) == 0
    L.wmar_vq_train_destroy(None)
