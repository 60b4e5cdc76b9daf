"""Every HMC kernel path against the float64 oracle (tests/hmc_cases.py lists the cases, the cells and the comparison).

Each case, in this order: (1) one call on the default stream inside a KernelProbe launched exactly the kernels
`expected_path` derives from the shape -- a change in dispatch fails the case instead of quietly testing another kernel;
(2) a burning and a Metropolis call against oracle.hmc.hmc_step with `compare`: the part of the move that comes from the
gradients, block by block, the energies, the decision and the returned q; (3) q and stats are views into larger buffers
and nothing around them, nor any input, changes; (4) a second call gives the same bits, and a chain run alone gives the
bits it gave among the others wherever the path and the slicing are the same; (5) sliced cases replay from a captured
graph on a side stream with the same bits, and the graph takes the next call's Philox step from device memory.
Beside the matrix, five consecutive Philox proposals of a sliced, a one-workgroup and a generic case, each compared
with the oracle started from the library's previous q."""

import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import hmc_cases as hc  # noqa: E402
from hmc_cases import CASES, CASE_BY_NAME, case_data, check_chains, compare, expected_path  # noqa: E402

SENTINEL = -12345.0
GUARD = 64
WORST = {}   # path -> (largest error / tolerance, case, quantity): printed at the end of the module


@pytest.fixture(scope="module")
def eng(gpu_device):
    found = sorted(k for k in os.environ if k.startswith("PYZ_HMC_"))
    if found:
        pytest.fail(f"{', '.join(found)} set in the environment: every expected launch of this module assumes the "
                    "defaults, and the cases set the per-call switches themselves -- unset them")
    from bayesian_inference_for_nn_amd import engine
    yield engine
    for path, (ratio, name, k) in sorted(WORST.items()):
        print(f"largest error / tolerance on the {path} path: {ratio:.3f} ({name}: {k})")


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def guarded(shape):
    """A contiguous view of `shape` inside a buffer filled with a sentinel: (buffer, view)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(*shape)


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


class Runner:
    """One plan and the device inputs of a case."""

    def __init__(self, eng, case, data):
        self.eng, self.case, self.data = eng, case, data
        spec = case.spec
        self.plan = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=case.rows, max_particles=case.P)
        self.x = dev(data.x)
        self.y = dev(data.y, torch.int32 if case.loss == "scce" else torch.float32)
        self.z = dev(data.z) if case.momentum == "injected" else None
        self.pm = dev(data.prior_mu) if case.vec_prior else None
        self.ps = dev(data.prior_sigma) if case.vec_prior else None
        self.inputs = [t.clone() for t in (self.x, self.y) + ((self.z,) if self.z is not None else ())]

    def inputs_unchanged(self):
        now = (self.x, self.y) + ((self.z,) if self.z is not None else ())
        return all(torch.equal(a, b) for a, b in zip(now, self.inputs))

    def call(self, q0, us, burning, step=None, chains=None, z=None, stream=None):
        """pyz_hmc_step on fresh guarded copies of q0 (all chains, or the listed ones): (q, stats) as numpy, guards checked."""
        case = self.case
        rows = slice(None) if chains is None else list(chains)
        q0 = np.ascontiguousarray(np.asarray(q0, dtype=np.float32)[rows])
        P = q0.shape[0]
        qbuf, q = guarded((P, case.D))
        sbuf, stats = guarded((P, 8))
        q.copy_(dev(q0))
        unit_p = None
        if z is not None:
            unit_p = dev(np.ascontiguousarray(z))
        elif self.z is not None:
            unit_p = self.z if chains is None else self.z[rows].contiguous()
        mu, sg = (0.0, 1.0) if case.vec_prior else (self.data.prior_mu, self.data.prior_sigma)
        us = list(np.asarray(us, dtype=np.float32)[rows])
        torch.cuda.synchronize()
        ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.default_stream())
        with ctx:
            self.plan.hmc_step(q, self.x, self.y, case.L, case.eps, case.m, mu, sg, us, case.step if step is None else step,
                               case.seed, stats, burning=burning, unit_p=unit_p, prior_mean_vec=self.pm, prior_sigma_vec=self.ps)
        (stream or torch.cuda.default_stream()).synchronize()
        torch.cuda.synchronize()
        assert guards_intact(qbuf), f"{case.name}: something outside q's {P} x {case.D} elements was written"
        assert guards_intact(sbuf), f"{case.name}: something outside stats' {P} x 8 elements was written"
        return q.cpu().numpy().copy(), stats.cpu().numpy().copy()

    def close(self):
        self.plan.close()


def chain_result(case, q0, z, burn, metro, c):
    """The compared quantities of chain c from the (q, stats) of a burning and of a Metropolis call."""
    (qb, sb), (qm, sm) = burn, metro
    keys = dict(U0=2, K0=3, U1=4, K1=5, log_ratio=6)
    return hc.result_from(case, q0, z, dict(q=qb[c], loss=sb[c, 1]),
                          dict(accepted=sm[c, 0] != 0.0, q=qm[c], loss=sm[c, 1], **{k: sm[c, i] for k, i in keys.items()}))


def note_worst(case, path, report):
    for k, (err, tol) in report.items():
        ratio = err / tol if tol > 0 else (0.0 if err == 0 else math.inf)
        print(f"{case.name}: {k}: error {err:.3e}, tolerance {tol:.3e}, ratio {ratio:.3f}")
        if ratio > WORST.get(path, (-1.0,))[0]:
            WORST[path] = (ratio, case.name, k)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


def set_env(monkeypatch, case):
    for k in hc.PER_CALL_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_hmc_case(eng, case, monkeypatch):
    set_env(monkeypatch, case)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    pa = expected_path(case, cu)
    data = case_data(case)
    us = hc.uniforms(case, data)
    run = Runner(eng, case, data)

    # 1. the launches (default stream: never captured; the probe launches eagerly)
    with eng.KernelProbe(2048) as kp:
        burn = run.call(data.q0, us, True)
    sites = tuple(n for n, _ in kp.launches if n in hc.HMC_SITES)
    print(case.name, pa.path, "NW", pa.NW, "launches", len(sites))
    assert sites == pa.launches, f"{case.name}: expected the {pa.path} path {pa.launches}, launched {sites}"

    # 2. against the oracle
    metro = run.call(data.q0, us, False)
    assert bool((burn[1][:, 0] == 1.0).all()), f"{case.name}: a burning call rejected a proposal"
    assert same_bits(burn[1][:, 2:7], metro[1][:, 2:7]), f"{case.name}: the energies of the burning and the Metropolis call differ"
    for c in check_chains(case.P):
        ref = hc.oracle_result(case, data, c)
        report = compare(chain_result(case, data.q0[c], data.z[c], burn, metro, c), ref, case, what=f"chain {c}: ")
        note_worst(case, pa.path, report)

    # 3. bounds (the guards around q and stats are checked by every call)
    assert run.inputs_unchanged(), f"{case.name}: x, y or unit_p changed"
    assert bool((metro[1][:, 7] == 0.0).all()) and bool((burn[1][:, 7] == 0.0).all()), f"{case.name}: stats[:, 7] != 0"

    # 4. determinism, and independence of the chains
    again = run.call(data.q0, us, False)
    assert same_bits(again[0], metro[0]) and same_bits(again[1], metro[1]), f"{case.name}: two calls from the same inputs differ"
    solo_path = expected_path(case, cu, P=1)
    for c in sorted({0, case.P - 1}) if case.P > 1 else []:
        if case.momentum == "philox" and c > 0:
            continue   # alone, a chain draws from chain 0's stream
        solo_b, solo_m = run.call(data.q0, us, True, chains=[c]), run.call(data.q0, us, False, chains=[c])
        if pa.path != "generic" and (solo_path.path, solo_path.NW) == (pa.path, pa.NW):
            assert same_bits(solo_m[0][0], metro[0][c]) and same_bits(solo_m[1][0], metro[1][c]) and \
                same_bits(solo_b[0][0], burn[0][c]), f"{case.name}: chain {c} alone differs from chain {c} of {case.P}"
        else:   # another kernel or another split of the sums: to the tolerance
            compare(chain_result(case, data.q0[c], data.z[c], solo_b, solo_m, 0), hc.oracle_result(case, data, c), case,
                    what=f"chain {c} alone: ")

    # 5. the graph of the sliced paths
    if pa.NW:
        side = torch.cuda.Stream()
        for k in range(2):   # capture, then replay
            g = run.call(data.q0, us, False, stream=side)
            assert same_bits(g[0], metro[0]) and same_bits(g[1], metro[1]), \
                f"{case.name}: side-stream call {k} differs from the default-stream call"
        nxt = run.call(data.q0, us, False, step=case.step + 1, stream=side)
        fresh = Runner(eng, case, data)
        want = fresh.call(data.q0, us, False, step=case.step + 1)
        fresh.close()
        assert same_bits(nxt[0], want[0]) and same_bits(nxt[1], want[1]), \
            f"{case.name}: the replayed graph did not take step {case.step + 1} from the call"
        if case.momentum == "philox":
            assert not same_bits(nxt[1][:, 3], metro[1][:, 3]), f"{case.name}: K0 did not change with the Philox step"
    run.close()


@pytest.mark.parametrize("name", ["res_b0_relu_c3", "fused_b1_relu_l20_philox", "gen_d255_fused_off"])
def test_five_consecutive_philox_proposals(eng, name, monkeypatch):
    """Each proposal against the oracle started from the library's previous q (errors do not compound into the
    tolerance); the third one is rejected, so the fourth starts from a restored q.  Every proposal has new inputs (q, the
    step's momentum): the float32 oracle's differences that set the tolerances are the largest over such a sequence
    (hmc_cases.sequence_rel32, CPU only)."""
    case = CASE_BY_NAME[name]
    assert case.momentum == "philox" and case.P <= 4
    set_env(monkeypatch, case)
    pa = expected_path(case, torch.cuda.get_device_properties(0).multi_processor_count)
    data = case_data(case)
    run = Runner(eng, case, data)
    q = data.q0.copy()
    rel32 = hc.sequence_rel32(case, 5)
    for k in range(5):
        step = case.step + k
        zs = np.stack([hc.philox_z(case, c, step=step) for c in range(case.P)])
        us = []
        for c in range(case.P):
            lr = hc.oracle_result(case, data, c, u=0.5, q=q[c], z=zs[c])["log_ratio"]
            ratio = math.exp(min(lr, 50.0))
            us.append(float(np.float32(2.0 * ratio + 0.1 if k == 2 else 0.5 * ratio)))
        burn = run.call(q, us, True, step=step)
        metro = run.call(q, us, False, step=step)
        refs = [hc.oracle_result(case, data, c, u=us[c], q=q[c], z=zs[c]) for c in range(case.P)]
        for c, ref in enumerate(refs):
            assert ref["accepted"] == (k != 2)
            note_worst(case, pa.path, compare(chain_result(case, q[c], zs[c], burn, metro, c), ref, case,
                                              what=f"proposal {k}, chain {c}: ", rel32=rel32))
        q = metro[0]
    run.close()
