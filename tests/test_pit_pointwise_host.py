"""CPU: the permutation-invariant l1 / mse entry points (csrc/loss.hip, sehip_pit_pointwise_*) are declared in include/sehip.h,
bound in sehip/_lib.py and exported; their argument validation runs before any HIP call; the block-count helper that sizes the
workspace is a host function; sehip.loss.pit_loss_pointwise exists.  The arithmetic is checked on the GPU in
tests/test_gpu_pit_pointwise.py."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("sehip_pit_pointwise_blocks", "sehip_pit_pointwise_fwd", "sehip_pit_pointwise_bwd")


def test_entry_points_declared_bound_and_exported():
    from sehip import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sehip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sehip_[a-z0-9_]+)\s*\(", text))
    lib = _lib.lib()
    for name in NEW_ENTRY_POINTS:
        assert name in declared and name in _lib.declared_symbols() and hasattr(lib, name), name


def test_block_count_helper_is_a_host_function():
    from sehip import _lib, ops
    lib = _lib.lib()
    assert lib.sehip_pit_pointwise_blocks(1, 2, 1, 1) == 1
    # one record per (b, c) row set and chunk of the row: more than one block per row from a few thousand samples on
    one_row = lib.sehip_pit_pointwise_blocks(1, 3, 1, 4096 + 5)
    assert one_row > 1 and lib.sehip_pit_pointwise_blocks(2, 3, 1, 4096 + 5) == 2 * one_row
    assert lib.sehip_pit_pointwise_blocks(3, 2, 2, 1003) % 6 == 0
    # the count does not depend on S (a block loads all S speakers), stays bounded for long rows and is at least B*C
    assert lib.sehip_pit_pointwise_blocks(32, 2, 1, 32000) == lib.sehip_pit_pointwise_blocks(32, 6, 1, 32000)
    assert 1 <= lib.sehip_pit_pointwise_blocks(1, 2, 1, 2 ** 30) <= 4096
    assert lib.sehip_pit_pointwise_blocks(5000, 2, 1, 7) == 5000
    for bad in ((0, 2, 1, 5), (1, 7, 1, 5), (1, 0, 1, 5), (1, 2, 0, 5), (1, 2, 1, 0)):
        assert lib.sehip_pit_pointwise_blocks(*bad) == 0, bad
        with pytest.raises(_lib.SehipError):
            ops.pit_pointwise_blocks(*bad)


def test_arguments_are_validated_before_any_hip_call():
    from sehip import _lib
    lib = _lib.lib()
    err = lambda: lib.sehip_last_error()
    fwd = lambda b, s, c, n, mode: lib.sehip_pit_pointwise_fwd(None, None, b, s, c, n, mode, None, None, None, None, None)
    bwd = lambda b, s, c, n, mode: lib.sehip_pit_pointwise_bwd(None, None, None, None, b, s, c, n, mode, None, None)
    for name, fn in (("fwd", fwd), ("bwd", bwd)):
        assert fn(2, 7, 1, 100, 0) != 0 and b"S=7" in err() and name.encode() in err()
        assert fn(2, 0, 1, 100, 0) != 0 and b"S=0" in err()
        assert fn(2, 2, 1, 100, 2) != 0 and b"mode=2" in err()
        assert fn(2, 2, 1, 0, 1) != 0 and b"n=0" in err()
        assert fn(0, 2, 1, 100, 1) != 0 and b"B=0" in err()
        assert fn(2, 2, 0, 100, 1) != 0 and b"C=0" in err()
        assert fn(2, 2, 1, 100, 1) != 0 and b"null pointer" in err()     # a valid shape still stops at the missing buffers
    with pytest.raises(_lib.SehipError):
        _lib.call("sehip_pit_pointwise_fwd", None, None, 2, 7, 1, 100, 0, None, None, None, None, None)


def test_python_layer_exists_and_refuses_the_cpu():
    import torch
    from sehip import loss as L
    from sehip._lib import SehipError
    assert callable(L.pit_loss_pointwise) and callable(L.pit_pointwise_workspace) and L.PIT_MAX_SPEAKERS == 6
    x = torch.zeros(2, 2, 1, 8)
    with pytest.raises(SehipError):                       # no CPU fallback: a missing GPU is an error
        L.pit_loss_pointwise(x, x, "mse")
    with pytest.raises(SehipError):
        L.pit_loss_pointwise(x, x[:, :1], "l1")           # shape mismatch
    with pytest.raises(SehipError):
        L.pit_loss_pointwise(x, x, "psa")
    with pytest.raises(SehipError):
        L.pit_loss_pointwise(torch.zeros(2, 7, 1, 8), torch.zeros(2, 7, 1, 8), "l1")
    assert "psa" in L.pit_loss.__doc__
