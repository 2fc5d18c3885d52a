"""The likelihood-model caches of skgpuppy_amd.Covariance are keyed on CONTENT: a model handed back by `_fitted_model_at` (the fused
Gaussian, Matern and periodic likelihoods), `_matrix_model_at` (the generic route) or `SPGPCovariance._fit_model` was built from what
(x, t, theta) hold NOW -- not from what the same Python object, or an earlier array at the same address, held at an earlier call -- and
the model it replaces is closed exactly once.

No GPU: the builders are stubs that count their calls and keep a copy of what they were given; nothing here touches the device (the
package imports once libgpx.so is built, as for the other *_model.py tests).

Before the content keys (x keyed by address or id()), these cases failed for both dense routes: in-place whole, in-place one entry,
recycled address, list, float32, view (a stale model came back) and equal content (a needless rebuild); the others passed."""
import numpy as np
import pytest

import importlib

C = importlib.import_module("skgpuppy_amd.Covariance")      # (the package exports the class of the same name over the module attribute)

N, D = 130, 3


class _Stub(object):
    """a device model's place: what it was built from, and how often it was closed"""

    def __init__(self, log, *seen):
        self.seen = tuple(None if a is None else np.array(a, copy=True) for a in seen)
        self.closed = 0
        log.append(self)

    def close(self):
        self.closed += 1


class _FittedRoute(object):
    """Covariance._fitted_model_at with a stub build(x, t, theta)"""
    name = "fitted"

    def __init__(self, monkeypatch):
        self.built = []
        self.fail_next = False
        self.cov = C.Covariance()

    def _build(self, x, t, th):
        if self.fail_next:
            self.fail_next = False
            raise np.linalg.LinAlgError("stub: not positive definite")
        return _Stub(self.built, x, t, th)

    def __call__(self, x, t, theta):
        return self.cov._fitted_model_at(x, t, theta, C._theta, self._build)

    def expected(self, x, t, theta):
        return (np.asarray(x, dtype=np.float64), np.asarray(t, dtype=np.float64), np.asarray(theta, dtype=np.float64))


class _CheapKernel(C.Covariance):
    """a generic operator whose cov_matrix is one NumPy expression of all of x and theta"""

    def cov_matrix(self, x, theta):
        a = np.asarray(x, dtype=np.float64)
        return np.exp(theta[0]) * (a @ a.T) + np.exp(theta[1]) * np.eye(a.shape[0])


class _MatrixRoute(object):
    """Covariance._matrix_model_at with _MatrixModel(K, t) replaced by the stub"""
    name = "matrix"

    def __init__(self, monkeypatch):
        self.built = []
        self.fail_next = False
        self.cov = _CheapKernel()
        monkeypatch.setattr(C, "_MatrixModel", self._build)

    def _build(self, K, t):
        if self.fail_next:
            self.fail_next = False
            raise np.linalg.LinAlgError("stub: not positive definite")
        return _Stub(self.built, K, t)

    def __call__(self, x, t, theta):
        return self.cov._matrix_model_at(x, t, theta)

    def expected(self, x, t, theta):
        return (self.cov.cov_matrix(x, theta), np.asarray(t, dtype=np.float64))


@pytest.fixture(params=[_FittedRoute, _MatrixRoute], ids=lambda r: r.name)
def route(request, monkeypatch):
    return request.param(monkeypatch)


def _data(seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (N, D)), rng.standard_normal(N), np.log(np.array([1.3, 0.01, 0.7, 1.1, 0.4]))


def _current(route, model, x, t, theta):
    """`model` is open, was built from the present content of (x, t, theta), and every model built before it was closed exactly once"""
    assert model is route.built[-1], "a model older than the newest build was served"
    for got, want in zip(model.seen, route.expected(x, t, theta)):
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), "the model served was built from other content"
    assert model.closed == 0
    assert [m.closed for m in route.built[:-1]] == [1] * (len(route.built) - 1)


def _edit_and_check(route, x, t, theta, edit, holder=None):
    """call, edit in place (`holder`: what is edited when x is a view or a derived object), call again: a second build, from the new content"""
    _current(route, route(x, t, theta), x, t, theta)
    assert len(route.built) == 1
    edit(x if holder is None else holder)
    _current(route, route(x, t, theta), x, t, theta)
    assert len(route.built) == 2


def test_x_overwritten_in_place(route):
    x, t, theta = _data()
    other = _data(1)[0]

    def edit(a):
        a[:] = other
    _edit_and_check(route, x, t, theta, edit)


def test_one_entry_of_x_changed(route):
    x, t, theta = _data()

    def edit(a):
        a[-1, -1] += 0.25
    _edit_and_check(route, x, t, theta, edit)


def test_temporaries_at_a_recycled_address(route):
    """for s in (1, 1.5, 2): f(x * s, t, theta) -- NumPy hands each same-shaped temporary the address of the one just freed"""
    x, t, theta = _data()
    scales = (1.0, 1.5, 2.0)
    kept = [x * s for s in scales]          # what each temporary holds, alive throughout: never at a temporary's address
    addresses, served = [], []

    def f(xs):
        addresses.append(xs.ctypes.data)
        served.append((route(xs, t, theta), len(route.built)))

    for s in scales:
        f(x * s)                            # the temporary goes when f returns
    if addresses[1] != addresses[0] and addresses[2] != addresses[1]:
        pytest.fail("the allocator recycled no address among the three temporaries %r: this run proves nothing" % (addresses,))
    for k, (model, nbuilt) in enumerate(served):
        assert nbuilt == k + 1, "s = %g was served from the cache" % scales[k]
        for got, want in zip(model.seen, route.expected(kept[k], t, theta)):
            assert got.tobytes() == want.tobytes(), "s = %g got a model built from other content" % scales[k]
    assert [m.closed for m in route.built] == [1, 1, 0]


def test_list_of_lists_edited_in_place(route):
    x, t, theta = _data()
    rows = x.tolist()

    def edit(r):
        r[-1][-1] += 0.25
        r[0] = [0.5, -0.5, 0.125]
    _edit_and_check(route, rows, t, theta, edit)


def test_float32_array_edited_in_place(route):
    x, t, theta = _data()
    x32 = x.astype(np.float32)

    def edit(a):
        a[N // 2, 1] += 0.25
    _edit_and_check(route, x32, t, theta, edit)


def test_view_whose_parent_is_edited(route):
    x, t, theta = _data()
    big = np.zeros((N, 2 * D))
    big[:, ::2] = x
    view = big[:, ::2]
    assert not view.flags.c_contiguous

    def edit(parent):
        parent[-1, -2] += 0.25          # the view's last row, last column
    _edit_and_check(route, view, t, theta, edit, holder=big)


def test_equal_content_in_two_arrays_is_one_build(route):
    x, t, theta = _data()
    first = route(x, t, theta)
    twin = x.copy()
    assert twin.ctypes.data != x.ctypes.data
    assert route(twin, t.copy(), theta.copy()) is first
    assert len(route.built) == 1 and first.closed == 0


def test_value_then_gradient_is_one_build(route):
    """what L-BFGS-B does at every step: two calls at the same (x, t, theta)"""
    x, t, theta = _data()
    first = route(x, t, theta)
    for _ in range(3):
        assert route(x, t, theta) is first
    assert len(route.built) == 1 and first.closed == 0
    _current(route, first, x, t, theta)


def test_t_or_theta_changed_alone_rebuilds(route):
    x, t, theta = _data()
    _current(route, route(x, t, theta), x, t, theta)
    t2 = t.copy()
    t2[-1] += 0.5
    _current(route, route(x, t2, theta), x, t2, theta)
    assert len(route.built) == 2
    th2 = theta.copy()
    th2[-1] += 0.1
    _current(route, route(x, t2, th2), x, t2, th2)
    assert len(route.built) == 3
    t2[0] -= 0.5                            # and t edited in place
    _current(route, route(x, t2, th2), x, t2, th2)
    assert len(route.built) == 4


def test_a_build_that_raises_leaves_no_closed_model_behind(route):
    x, t, theta = _data()
    first = route(x, t, theta)
    th2 = theta.copy()
    th2[0] += 0.5
    route.fail_next = True
    with pytest.raises(np.linalg.LinAlgError):
        route(x, t, th2)
    assert first.closed == 1 and len(route.built) == 1
    again = route(x, t, theta)              # the closed model is not served: a new build, also at the old key
    assert again is not first and len(route.built) == 2
    _current(route, again, x, t, theta)
    assert first.closed == 1


class _NameKernel(C.Covariance):
    """a kernel on rows that are no numbers"""

    def cov_matrix(self, x, theta):
        v = np.array([float(sum(len(s) for s in row)) for row in x])
        return np.exp(theta[0]) * np.outer(v, v) + np.eye(len(x))


def test_non_numeric_x_is_never_served_from_a_cache(monkeypatch):
    route = _MatrixRoute(monkeypatch)
    route.cov = _NameKernel()
    x = [("ab", "c"), ("d", "efg"), ("hi", "jk")]
    t, theta = np.array([0.5, -0.25, 1.0]), np.array([0.1])
    _current(route, route(x, t, theta), x, t, theta)
    x[-1] = ("hijklm", "n")                 # the list keeps its id
    _current(route, route(x, t, theta), x, t, theta)
    assert len(route.built) == 2
    _current(route, route(x, t, theta), x, t, theta)
    assert len(route.built) == 3            # rebuilt at every call: the accepted cost of having no content key


def test_spgp_fit_model_sees_an_in_place_edit():
    m = 4
    cov = C.SPGPCovariance(m)
    built = []
    cov._model = lambda x, t, theta: _Stub(built, x, t, theta)
    x, t, _ = _data()
    theta = np.concatenate([np.log(np.array([1.3, 0.01, 0.7, 1.1, 0.4])), x[:m].ravel()])
    first = cov._fit_model(x, t, theta)
    assert cov._fit_model(x, t, theta) is first and len(built) == 1
    assert cov._fit_model(x.copy(), t.copy(), theta.copy()) is first and len(built) == 1
    x[-1, -1] += 0.25
    second = cov._fit_model(x, t, theta)
    assert second is not first and len(built) == 2 and first.closed == 1 and second.closed == 0
    assert second.seen[0].tobytes() == x.tobytes()
    x[:] = _data(1)[0]
    third = cov._fit_model(x, t, theta)
    assert len(built) == 3 and [b.closed for b in built] == [1, 1, 0]
    assert third.seen[0].tobytes() == x.tobytes()
