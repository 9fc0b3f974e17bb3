"""CPU: the host model of spmv_hip_cg_mixed (tests/cg_mixed_cases.py) alone, on cg_cases' matrices with cg_cases.matvec.

What the GPU tests take for granted is shown here: that the recurrence of the contract reaches an fp64 answer with fp32 iterations where the
fp32 solve cannot, at a cost in iterations that stays small, and that every segment end and status of the contract is reached by a named case."""
import numpy as np
import pytest

import cg_cases as cgc
import cg_mixed_cases as mix

RTOL = 1e-12
SYSTEMS = {"lap2d32": lambda: cgc.lap2d(32), "tri1025": lambda: cgc.tri(1025), "dominant2049": lambda: cgc.dominant(2049)}


@pytest.fixture(scope="module")
def solved():
    """name -> (matrix, b, the mixed model's run, the fp64 model's run), computed once"""
    out = {}
    for name, make in SYSTEMS.items():
        csr = make()
        b = cgc.rhs(csr.m, np.float64)
        high, low = mix.callbacks(csr)
        out[name] = (csr, b, mix.cg_mixed(high, low, b, rtol=RTOL, max_iterations=5000), cgc.cg(high, b, rtol=RTOL, max_iterations=5000))
    return out


@pytest.mark.parametrize("name", SYSTEMS)
def test_the_model_converges_to_an_fp64_answer(solved, name):
    csr, b, run, _ = solved[name]
    true = cgc.true_residual(csr, b, run["x"])
    print(f"{name}: {run['iterations']} iterations, {run['updates']} updates, true residual {true:.3e}, segments {run['segments']}")
    assert run["status"] == mix.CONVERGED
    assert run["x"].dtype == np.float64
    assert true <= 2 * RTOL          # the factor 2: the rounding of the multiply that recomputes it
    assert run["rr"] <= RTOL * RTOL * run["bb"]


@pytest.mark.parametrize("name", SYSTEMS)
def test_the_fp32_solve_stops_far_above_it(name):
    csr = SYSTEMS[name]()
    b = cgc.rhs(csr.m, np.float64)
    run = cgc.cg(cgc.matvec(csr, np.float32), b.astype(np.float32), rtol=RTOL, max_iterations=5000)
    true = cgc.true_residual(csr, b, run["x"])
    print(f"{name}: fp32 CG ends with status {run['status']} after {run['iterations']} iterations, true residual {true:.3e}")
    assert true > 1e-7


@pytest.mark.parametrize("name", SYSTEMS)
def test_keeping_the_direction_costs_few_iterations(solved, name):
    _, _, run, ref = solved[name]
    assert ref["status"] == cgc.CONVERGED
    print(f"{name}: mixed {run['iterations']} iterations, fp64 {ref['iterations']}: {run['iterations'] / ref['iterations']:.2f}")
    assert run["iterations"] <= 1.5 * ref["iterations"]


@pytest.mark.parametrize("name", mix.named_cases())
def test_every_segment_end_and_status_has_its_case(name):
    hi, lo, b, kw, status, what = mix.named_cases()[name]
    run = mix.cg_mixed(cgc.matvec(hi), cgc.matvec(lo), b, **kw)
    print(f"{name}: status {run['status']}, end {run['end']}, {run['iterations']} iterations, {run['updates']} updates, segments {run['segments']}")
    assert run["status"] == status
    assert what in run["segments"] or what == run["end"]
    if name == "exact":          # a fresh direction follows: the next segment's first alpha is rz / <z, A z> again, and it ends exact too
        assert run["segments"][:2] == ["exact", "exact"] and run["updates"] >= 2
    if status in (mix.BREAKDOWN, mix.NONFINITE, mix.STAGNATED):
        assert run["end"] == what
    if name == "stagnated":      # the rejected update is not counted, x and rr are the last committed ones
        assert run["updates"] == 0 and not run["x"].any() and run["rr"] == run["history"][0]
    if name == "breakdown":
        assert np.isfinite(run["x"]).all()


def test_history_follows_its_rules():
    csr = cgc.lap2d(12)
    b = cgc.rhs(csr.m, np.float64, 3)
    high, low = mix.callbacks(csr)
    run = mix.cg_mixed(high, low, b, rtol=1e-12, max_iterations=500, update_every=4)
    h = run["history"]
    assert run["status"] == mix.CONVERGED and h.size == run["iterations"] + 1 and run["updates"] == len(run["segments"])
    assert h[0] == cgc.dot(b, b) == run["bb"]                        # x0 = 0: r64 = b
    assert h[-1] == run["rr"]                                         # the last update's true rr
    # behind each of the first updates stands the true rr of the iterate that the update committed
    k = 0
    for reason in run["segments"][:3]:
        k = k + 4 if reason == "every" else None
        if k is None:
            break
        r = b - high(run["iterates"][k])
        assert h[k] == cgc.dot(r, r)


def test_a_budget_returns_what_a_longer_run_held_plus_one_update():
    csr = cgc.tri(1025)
    b = cgc.rhs(csr.m, np.float64)
    high, low = mix.callbacks(csr)
    kw = dict(rtol=0.0, update_drop=0.5, update_every=2)
    long = mix.cg_mixed(high, low, b, max_iterations=9, **kw)
    for k in (1, 2, 5, 9):
        short = mix.cg_mixed(high, low, b, max_iterations=k, **kw)
        assert (short["status"], short["iterations"]) == (mix.MAX_ITERATIONS, k)
        assert short["x"].tobytes() == long["iterates"][k].tobytes()
        assert short["history"][:k].tobytes() == long["history"][:k].tobytes()
    zero = mix.cg_mixed(high, low, b, max_iterations=0, **kw)
    assert (zero["status"], zero["iterations"], zero["updates"]) == (mix.MAX_ITERATIONS, 0, 0) and not zero["x"].any()


def test_dinv_of_ones_changes_no_bit_and_jacobi_helps_on_the_scaled_laplacian():
    csr = cgc.scaled(12)
    b = cgc.rhs(csr.m, np.float64)
    high, low = mix.callbacks(csr)
    plain = mix.cg_mixed(high, low, b, rtol=1e-10, max_iterations=20000)
    ones = mix.cg_mixed(high, low, b, rtol=1e-10, max_iterations=20000, dinv=np.ones(csr.m, dtype=np.float32))
    jac = mix.cg_mixed(high, low, b, rtol=1e-10, max_iterations=20000, dinv=(1.0 / cgc.diagonal(csr)).astype(np.float32))
    assert plain["x"].tobytes() == ones["x"].tobytes() and plain["history"].tobytes() == ones["history"].tobytes()
    assert plain["status"] == jac["status"] == mix.CONVERGED and jac["iterations"] < plain["iterations"]
