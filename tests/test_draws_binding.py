"""The argument rules of host/draws.py and the context manager of companion.Handle, on CPU tensors: no library, no device. The handle's
device is a parameter of every rule, so torch.device("cpu") stands in for it. The error texts are written out: they are part of the interface."""
import ctypes as C
import importlib

import pytest
import torch

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def draws(pkg):
    return importlib.import_module(pkg.__name__ + ".host.draws")


@pytest.fixture(scope="module")
def companion(pkg):
    return importlib.import_module(pkg.__name__ + ".host.companion")


def f64(*shape):
    return torch.zeros(shape, dtype=torch.float64)


# ---- chain_matrix
def test_chain_matrix_contiguous(draws):
    assert draws.chain_matrix(f64(3, 5), 3, CPU, "lbfgs") == (3, 5, 5)


def test_chain_matrix_view_of_a_wider_buffer(draws):
    assert draws.chain_matrix(f64(3, 8)[:, :5], 3, CPU, "lbfgs") == (3, 5, 8)


def test_chain_matrix_without_columns(draws):
    assert draws.chain_matrix(f64(3, 0), 3, CPU, "lbfgs") == (3, 0, 0)


def test_chain_matrix_single_row_ignores_its_stride(draws):
    x = f64(2, 8)[:1, :5]
    assert x.stride(0) == 8
    assert draws.chain_matrix(x, 1, CPU, "lbfgs") == (1, 5, 5)


def test_chain_matrix_any_row_count(draws):
    assert draws.chain_matrix(f64(2, 4), None, CPU, "moments", "x") == (2, 4, 4)
    assert draws.chain_matrix(f64(2, 6)[:, :4], None, CPU, "moments", "x") == (2, 4, 6)
    assert draws.chain_matrix(f64(1, 4), None, CPU, "moments", "x") == (1, 4, 4)
    assert draws.chain_matrix(f64(2, 6)[:1, :4], None, CPU, "moments", "x") == (1, 4, 4)


@pytest.mark.parametrize("x, rows, dev, what, name, message", [
    (torch.zeros((3, 5), dtype=torch.float32), 3, CPU, "lbfgs", "theta_t",
     "lbfgs: theta_t must be a float64 [D = 3, W] tensor on cpu with contiguous rows"),
    (f64(5), None, CPU, "moments", "x", "moments: x must be a float64 [K, W] tensor on cpu with contiguous rows"),
    (f64(5), 3, CPU, "pathfinder_draw", "theta_t", "pathfinder_draw: theta_t must be a float64 [D = 3, W] tensor on cpu with contiguous rows"),
    (f64(4, 5), 3, CPU, "pathfinder", "theta_t", "pathfinder: theta_t must be a float64 [D = 3, W] tensor on cpu with contiguous rows"),
    (f64(5, 3).t(), 3, CPU, "lbfgs_direction", "g", "lbfgs_direction: g must be a float64 [D = 3, W] tensor on cpu with contiguous rows"),
    (f64(5, 3).t(), None, CPU, "chain_moments", "cmean", "chain_moments: cmean must be a float64 [K, W] tensor on cpu with contiguous rows"),
    (f64(3, 5), 3, torch.device("cuda", 0), "hmc_step", "theta_t",
     "hmc_step: theta_t must be a float64 [D = 3, W] tensor on cuda:0 with contiguous rows"),
], ids=["float32", "one-dimensional", "one-dimensional-D", "row-count", "transposed", "transposed-K", "other-device"])
def test_chain_matrix_refuses(draws, x, rows, dev, what, name, message):
    with pytest.raises(ValueError) as e:
        draws.chain_matrix(x, rows, dev, what, name)
    assert str(e.value) == message


# ---- slot-major stacks [n, D, W] and the history that holds two of them
def stack(n, D, W, ld):
    return f64(n, D, ld)[:, :, :W]


def counts(W):
    return torch.ones(W, dtype=torch.int64), torch.zeros(W, dtype=torch.int64)


def test_history_with_a_padded_leading_dimension(draws):
    cnt, head = counts(4)
    W, ld, m, c, h = draws.history(cnt, head, stack(2, 3, 4, 6), stack(2, 3, 4, 6), f64(3, 6)[:, :4], 3, CPU, "lbfgs_direction")
    assert (W, ld, m) == (4, 6, 2)
    assert c.dtype == h.dtype == torch.int32 and c.shape == h.shape == (4,) and c.is_contiguous() and h.is_contiguous()


def test_history_refuses_rows_of_another_leading_dimension(draws):
    cnt, head = counts(4)
    with pytest.raises(ValueError) as e:
        draws.history(cnt, head, stack(2, 3, 4, 6), stack(2, 3, 4, 4), f64(3, 6)[:, :4], 3, CPU, "lbfgs_direction")
    assert str(e.value) == "lbfgs_direction: Y must be a float64 [m, D = 3, W = 4] tensor on cpu with g's leading dimension"
    with pytest.raises(ValueError) as e:
        draws.history(cnt, head, stack(2, 3, 4, 4), stack(2, 3, 4, 6), f64(3, 6)[:, :4], 3, CPU, "pathfinder_fit")
    assert str(e.value) == "pathfinder_fit: S must be a float64 [m, D = 3, W = 4] tensor on cpu with g's leading dimension"


def test_history_of_single_rows_takes_the_slot_distance_of_S(draws):
    cnt, head = counts(4)
    S = stack(2, 1, 4, 6)
    assert S.stride(0) == 6
    assert draws.history(cnt, head, S, stack(2, 1, 4, 6), f64(1, 4), 1, CPU, "lbfgs_direction")[:3] == (4, 6, 2)
    with pytest.raises(ValueError):      # … and Y has to agree with it
        draws.history(cnt, head, S, stack(2, 1, 4, 5), f64(1, 4), 1, CPU, "lbfgs_direction")


def test_single_rows_and_a_single_slot_take_the_distance_of_the_draws(draws):
    S, z = stack(1, 1, 4, 6), stack(3, 1, 4, 7)
    assert draws.single_row_ld(4, 1, (S, 1), (z, 3)) == 7
    assert draws.single_row_ld(4, 1, (stack(2, 1, 4, 6), 2), (z, 3)) == 6      # S before z
    assert draws.single_row_ld(4, 1, (S, 1), (z[:1], 1)) == 4
    assert draws.single_row_ld(5, 3, (stack(2, 3, 4, 6), 2), (z, 3)) == 5      # more than one row: the matrix says it
    draws.slot_stack(z, 3, 1, 4, 7, CPU, "pathfinder_fit", "z", slots="n")
    with pytest.raises(ValueError) as e:
        draws.slot_stack(z, 3, 1, 4, 6, CPU, "pathfinder_fit", "z", slots="n")
    assert str(e.value) == "pathfinder_fit: z must be a float64 [n, D = 1, W = 4] tensor on cpu with g's leading dimension"


def test_history_refuses_counts_of_another_length(draws):
    cnt, head = counts(4)
    with pytest.raises(ValueError) as e:
        draws.history(cnt[:3], head, stack(2, 3, 4, 6), stack(2, 3, 4, 6), f64(3, 6)[:, :4], 3, CPU, "lbfgs_direction")
    assert str(e.value) == "lbfgs_direction: cnt and head take 4 values each"


# ---- vectors, group ids, the dual-averaging state, pointers
def test_device_vector(draws):
    v = draws.device_vector(0.5, 3, CPU, "eps")
    assert v.dtype == torch.float64 and v.is_contiguous() and v.tolist() == [0.5, 0.5, 0.5]
    assert draws.device_vector([1.0, 2.0, 3.0], 3, CPU, "eps").tolist() == [1.0, 2.0, 3.0]
    assert draws.device_vector(None, 3, CPU, "eps") is None
    with pytest.raises(ValueError) as e:
        draws.device_vector([1.0, 2.0], 3, CPU, "eps")
    assert str(e.value) == "eps: expected 3 values, got a tensor of shape (2,)"


def test_group_ids(draws):
    g = draws.group_ids(torch.arange(8, dtype=torch.int64)[::2], 4, CPU, "moments")
    assert g.dtype == torch.int32 and g.is_contiguous() and g.tolist() == [0, 2, 4, 6]
    assert draws.group_ids(None, 4, CPU, "moments") is None
    with pytest.raises(ValueError) as e:
        draws.group_ids(torch.arange(3), 4, CPU, "moments")
    assert str(e.value) == "moments: group takes 4 ids"


def test_adapt_state(draws):
    assert draws.is_adapt_state(f64(2, 4), 2, CPU)
    assert not draws.is_adapt_state(f64(2, 3), 2, CPU)
    assert not draws.is_adapt_state(torch.zeros((2, 4), dtype=torch.float32), 2, CPU)
    assert not draws.is_adapt_state(f64(2, 8)[:, ::2], 2, CPU)
    assert not draws.is_adapt_state(f64(2, 4), 2, torch.device("cuda", 0))


def test_ptr(draws):
    x = f64(3)
    assert draws.ptr(None) is None and draws.ptr(x) == x.data_ptr()


# ---- companion.Handle as a context manager
class RecordingLib:
    def __init__(self):
        self.calls = []

    def octo_stub_destroy(self, h):
        self.calls.append(("destroy", h.value))


@pytest.fixture
def stub_handle(companion):
    class Stub(companion.Handle):
        PREFIX = "octo_stub"

        def __init__(self, lib):
            self._open(lib, 0)
            self._h = C.c_void_p(1234)
    return Stub


def test_handle_with_closes_once(stub_handle):
    lib = RecordingLib()
    with stub_handle(lib) as h:
        assert isinstance(h, stub_handle) and lib.calls == []
    assert lib.calls == [("destroy", 1234)] and h._h is None
    h.close()
    del h
    assert lib.calls == [("destroy", 1234)]


def test_handle_with_closes_once_when_the_body_raises(stub_handle):
    lib = RecordingLib()
    with pytest.raises(KeyError, match="from the body"):
        with stub_handle(lib):
            raise KeyError("from the body")
    assert lib.calls == [("destroy", 1234)]
