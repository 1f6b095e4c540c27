"""CPU: the Chamfer entry points of the C ABI validate their arguments before any launch, and
the Python layers above them have no CPU path."""
import pytest
import torch

import kdpc_native

EINVAL = 1  # hipErrorInvalidValue
P = 0x1000  # a non-null pointer value: never dereferenced, every call below returns first


def _fwd(lib, b, n, m, ptrs=(P,) * 6):
    return lib.kdpc_chamfer_fwd(b, n, m, *ptrs, None)


def _bwd(lib, b, n, m, ptrs=(P,) * 8):
    """ptrs = (a, bp, idx_ab, g_ab, offsets_ba, perm_ba, g_ba, da)."""
    return lib.kdpc_chamfer_bwd(b, n, m, *ptrs, None)


@pytest.mark.parametrize("b,n,m", [(1, 0, 5), (1, 5, 0), (65536, 5, 5), (-1, 5, 5),
                                   (65535, 40000, 5), (65535, 5, 40000)])
def test_invalid_sizes_rejected_without_launch(b, n, m):
    lib = kdpc_native.load_library()
    assert _fwd(lib, b, n, m) == EINVAL
    assert _bwd(lib, b, n, m) == EINVAL
    assert _bwd(lib, b, n, m, (P, P, P, P, None, None, None, P)) == EINVAL


def test_empty_batch_is_a_successful_noop():
    lib = kdpc_native.load_library()
    assert _fwd(lib, 0, 5, 7) == 0
    assert _fwd(lib, 0, 5, 7, (None,) * 6) == 0
    assert _bwd(lib, 0, 5, 7) == 0
    assert _bwd(lib, 0, 5, 7, (None,) * 8) == 0


@pytest.mark.parametrize("null", range(6))
def test_fwd_null_buffers_rejected(null):
    lib = kdpc_native.load_library()
    ptrs = [P] * 6
    ptrs[null] = None
    assert _fwd(lib, 2, 5, 7, ptrs) == EINVAL


@pytest.mark.parametrize("null", [0, 1, 2, 3, 7])
@pytest.mark.parametrize("two", [True, False])
def test_bwd_null_buffers_rejected(null, two):
    lib = kdpc_native.load_library()
    ptrs = [P] * 8 if two else [P, P, P, P, None, None, None, P]
    ptrs[null] = None
    assert _bwd(lib, 2, 5, 7, ptrs) == EINVAL


@pytest.mark.parametrize("given", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1),
                                   (0, 1, 1)])
def test_bwd_partial_ba_set_rejected(given):
    """g_ba, offsets_ba and perm_ba are NULL together or not at all."""
    lib = kdpc_native.load_library()
    ptrs = [P, P, P, P] + [P if g else None for g in given] + [P]
    assert _bwd(lib, 2, 5, 7, ptrs) == EINVAL
    assert _bwd(lib, 0, 5, 7, ptrs) == EINVAL  # whatever the batch size


def test_no_cpu_path():
    import selfsup
    a, b = torch.zeros(1, 4, 3), torch.zeros(1, 5, 3)
    with pytest.raises(kdpc_native.KdpcError):
        kdpc_native.chamfer_fwd(a, b)
    with pytest.raises(kdpc_native.KdpcError):
        kdpc_native.chamfer_bwd(a, b, torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 4))
    with pytest.raises(kdpc_native.KdpcError):
        selfsup.chamfer_distance(a, b)
    with pytest.raises(kdpc_native.KdpcError):
        selfsup.chamfer_distance(a.requires_grad_(), b)
    ops = kdpc_native.load_ops()
    with pytest.raises(NotImplementedError):  # no CPU kernel is registered
        torch.ops.kdpc_selfsup.chamfer_fwd(a.detach(), b)
    assert ops is torch.ops.kdpc


def test_train_steps_are_exported():
    import distill
    import selfsup
    assert distill.SelfSupTrainStep(None, None).loss_fn is selfsup.multiScaleChamferSmooth
    assert callable(distill.graphed_selfsup_step)
