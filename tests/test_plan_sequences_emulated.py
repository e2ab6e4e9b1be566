"""Call sequences on one live plan against fresh plans (plan_sequence_common.py has the catalogue, the two judgements and the
sequences) on the CPU emulation of the HIP runtime (tests/emu), both precisions, nfft = 2^15:

  (a) one argument changes          every entry point: E(A), E(one argument changed), E(A), for every argument it has
  (b) all ordered pairs             an Euler walk over the entry points: every ordered pair consecutively (asserted, not sampled);
                                    the Bluestein calls in a walk of their own, mixed with power-of-two calls on the same plan
  (c) eviction                      five grids on four slots, with the slot's derived copies (pool_dev, adj_dev) the freshest thing
                                    in it; the calls back to back; once more under the emulator's `waves-reverse` schedule
  (d) invalidation                  the walk of (b) with a change of the tolerance, or of one of four options, before every 7th
                                    call, away and back in turn, and the return to the first state
  (e) scratch order                 small-large-small and large-small-large in n0, rows and nbatch, one at a time
  (f) refused calls                 the walk of (b) with one refused call between any two: the calls after it keep their bits,
                                    last_split() stays; the refusal that takes a slot before it refuses, placed on purpose
  (g) seeded walks                  three seeds x 40 steps over entry points x grids A ... E x two n0, tolerance and options included

and, at the Python level, the shim's own caches: a fixed sequence through the public API, every result and gradient equal in bits
to the same call as the first call of a fresh engine set.

(d) and (f) run over the whole walk of (b).  The grids of (a) that differ in the first or in the last scale are there because a
key that loses an END of the scales array collides on nothing else: the row count is in the head of the key.
"""
import numpy as np
import pytest

import plan_sequence_common as ps
import pycwt_amd
from test_emu_schedules import WAVES_REVERSE, schedule  # noqa: F401  (the fixture that sets and restores the emulator's schedule)
from test_kernels_emulated import TOL

N = 1 << ps.LOGN
PRECS = [64, 32]
_runners = {}


def runner(lib, prec):
    """one per precision for the whole module: the fresh plans' results are memoised in it"""
    if prec not in _runners:
        _runners[prec] = ps.Runner(lib, N, prec, TOL)
    return _runners[prec]


# ---- structure ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_the_grids_hold_every_form(emu_library, prec):
    """ROWS is the floor: grid A has narrow, overlap-save, band-passed and polynomial rows, grid E (two rows clipped at Nyquist,
    too few for the band-passed form) the two-pass rows -- one grid cannot hold both: the band-passed form is decided per call"""
    a, e = ps.base_split(emu_library, N, prec), ps.base_split(emu_library, N, prec, name="E")
    assert all(a[f] > 0 for f in ("narrow", "ols", "aols", "poly")), a
    assert e["two_pass"] > 0, e


def test_every_entry_point_is_in_a_sequence_and_every_ordered_pair_in_the_walk():
    in_a = {s.entry for e in ps.NAMES for s in ps.seq_one_argument(e)}
    assert in_a == set(ps.NAMES)
    walk = [c.entry for c in ps.seq_pairs()]
    assert ps.pairs_of(walk) == {(a, b) for a in ps.POW2_NAMES for b in ps.POW2_NAMES} and len(walk) == len(ps.POW2_NAMES) ** 2 + 1
    assert set(ps.REFUSALS) == {s.name for s in ps.seq_refusals() if isinstance(s, ps.Refused)}


# ---- (a) -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("entry", ps.NAMES)
def test_a_one_argument_changes(emu_library, entry, prec):
    """The collisions a flat concatenated key can get wrong: the same scales with one other argument changed, and grids that
    differ in one scale at the start, in the middle or at the end of the array, in order or in length."""
    runner(emu_library, prec).run(ps.seq_one_argument(entry), "(a) " + entry)


# ---- (b) -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_b_all_ordered_pairs(emu_library, prec):
    made = runner(emu_library, prec).run(ps.seq_pairs(), "(b)")
    assert made == len(ps.POW2_NAMES) ** 2 + 1


@pytest.mark.parametrize("prec", PRECS)
def test_b_bluestein_between_power_of_two_calls(emu_library, prec):
    """nfft = 2^15 >= 2 n0 - 1 for both Bluestein lengths: every ordered pair of BLUESTEIN_MIX (plan_sequence_common), then the other length"""
    steps = ps.seq_pairs(ps.BLUESTEIN_MIX)
    steps += [ps.Call("bluestein", n0="small"), ps.Call("transform"), ps.Call("bluestein"), ps.Call("bluestein", n0="small")]
    runner(emu_library, prec).run(steps, "(b) bluestein")


# ---- (c) -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("derived,other", ps.EVICTION_PAIRS)
def test_c_eviction_with_derived_copies_pending(emu_library, derived, other, prec):
    """With pool_dense left at its old value in upload_row_table a pooled call on a rebuilt slot reads the rank map of the table
    that had the slot before."""
    for k, steps in enumerate(ps.seq_eviction(derived, other)):
        runner(emu_library, prec).run(steps, "(c) %s / %s, sequence %d" % (derived, other, k), back_to_back=True)


@pytest.mark.parametrize("prec", PRECS)
def test_c_eviction_under_the_reverse_wave_schedule(emu_library, schedule, prec):  # noqa: F811
    schedule(WAVES_REVERSE)
    for k, steps in enumerate(ps.seq_eviction(*ps.EVICTION_PAIRS[0])):
        runner(emu_library, prec).run(steps, "(c) waves-reverse, sequence %d" % k, back_to_back=True)


# ---- (d) -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("toggle", ps.TOGGLES)
def test_d_invalidation(emu_library, toggle, prec):
    """Without the loop that clears the keys in cwt_plan_set_option the calls after `poly = 0` run the polynomial tables of
    before."""
    runner(emu_library, prec).run(ps.seq_invalidation(toggle, prec), "(d) " + toggle)


# ---- (e) -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("entry", list(ps.SCRATCH))
def test_e_scratch_order(emu_library, entry, prec):
    for dim, up, down in ps.seq_scratch(entry):
        runner(emu_library, prec).run(up, "(e) %s, %s: small-large-small" % (entry, dim))
        runner(emu_library, prec).run(down, "(e) %s, %s: large-small-large" % (entry, dim))


@pytest.mark.parametrize("prec", PRECS)
def test_e_execute_host_at_two_lengths(emu_library, prec):
    """the host staging of cwt_execute_host sized by a short call and then used by a long one, and the reverse, between device calls"""
    small, big = ps.Call("execute_host", n0="small"), ps.Call("execute_host")
    for steps in ([small, big, ps.Call("execute_host_power", n0="small"), ps.Call("transform"), big],
                  [big, small, ps.Call("execute_host_power"), ps.Call("transform_pool"), small]):
        runner(emu_library, prec).run(steps, "(e) execute_host")


# ---- (f) -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_f_refused_calls_leave_no_trace(emu_library, prec):
    runner(emu_library, prec).run(ps.seq_refusals(), "(f)")


@pytest.mark.parametrize("prec", PRECS)
def test_f_refusal_that_has_taken_a_slot(emu_library, prec):
    runner(emu_library, prec).run(ps.seq_refusal_after_lookup(), "(f) a scale of 0")


# ---- (g) -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("seed", ps.SEEDS)
def test_g_seeded_walks(emu_library, seed, prec):
    runner(emu_library, prec).run(ps.seq_walk(seed, prec), "(g) seed %d" % seed)


# ---- the shim's own caches -------------------------------------------------------------------------------------------------------------
def _arrays(out):
    """every array of a result, as NumPy"""
    if isinstance(out, (tuple, list)):
        return [a for o in out for a in _arrays(o)]
    if out is None:
        return []
    if hasattr(out, "detach"):
        return [out.detach().cpu().numpy()]
    return [np.asarray(out)]


def _shim_ops():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(41)
    x1, y1 = rng.standard_normal(3000), rng.standard_normal(3000)          # 3000 and 3500 share the padded length 4096 ...
    x2 = rng.standard_normal(3500)
    x3 = rng.standard_normal(5000)                                         # ... 5000 pads to 8192
    X = rng.standard_normal((3, 3000))
    sc = np.geomspace(2.0, 600.0, 12)

    def torch_grad(fn, x, **kw):
        def op():
            t = torch.as_tensor(x).clone().requires_grad_(True)
            extra = {k: v.clone().requires_grad_(True) for k, v in kw.items()}
            out = fn(t, 0.5, **extra)[0] if extra else fn(t, 0.5, 1 / 4)[0]
            (out.abs() ** 2).sum().backward()
            return [out, t.grad] + [v.grad for v in extra.values()]
        return op

    def device_icwt():
        d = pycwt_amd.cwt_device(x1, 0.5, 1 / 4)
        try:
            return [d.W(), d.icwt(1 / 4)]
        finally:
            d.close()
    scales_f0 = dict(scales=torch.as_tensor(sc), f0=torch.tensor(6.0, dtype=torch.float64))
    return [
        ("cwt", lambda: pycwt_amd.cwt(x1, 0.5, 1 / 4)),
        ("cwt_power pool", lambda: pycwt_amd.cwt_power(x1, 0.5, 1 / 4, pool=16)),
        ("cwt_power hop, the other length", lambda: pycwt_amd.cwt_power(x2, 0.5, 1 / 4, hop=16)),
        ("xwt", lambda: pycwt_amd.xwt(x1, y1, 0.5, 1 / 4)),
        ("release_scratch", pycwt_amd.release_scratch),
        ("wct", lambda: pycwt_amd.wct(x1, y1, 0.5, 1 / 4, sig=False)),
        ("cwt_device + icwt", device_icwt),
        ("cwt_batch", lambda: pycwt_amd.cwt_batch(X, 0.5, 1 / 4)),
        ("set_tolerance 1e-9", lambda: pycwt_amd.set_tolerance(1e-9)),
        ("cwt at 1e-9", lambda: pycwt_amd.cwt(x1, 0.5, 1 / 4)),
        ("cwt_torch at 1e-9", torch_grad(pycwt_amd.cwt_torch, x2)),
        ("set_tolerance back", lambda: pycwt_amd.set_tolerance(None)),
        ("cwt_torch", torch_grad(pycwt_amd.cwt_torch, x1)),
        ("cwt_power_torch pool", torch_grad(lambda t, dt, dj: pycwt_amd.cwt_power_torch(t, dt, dj, pool=16), x1)),
        ("release_scratch", pycwt_amd.release_scratch),
        ("cwt_torch scales f0", torch_grad(pycwt_amd.cwt_torch, x2, **scales_f0)),
        ("cwt, the longer padded length", lambda: pycwt_amd.cwt(x3, 0.5, 1 / 4, wavelet="dog")),
        ("cwt pad=False", lambda: pycwt_amd.cwt(x3, 0.5, 1 / 4, pad=False)),
        ("cwt again", lambda: pycwt_amd.cwt(x1, 0.5, 1 / 4)),
        ("cwt_power pool again", lambda: pycwt_amd.cwt_power(x2, 0.5, 1 / 4, pool=16)),
    ]


SETTINGS = ("set_tolerance 1e-9", "set_tolerance back", "release_scratch")


def test_shim_caches_against_fresh_engines(emulated, monkeypatch):
    """One plan per (length, precision) in pycwt_amd.wavelet, one engine per (length, precision) in pycwt_amd.autograd, the pool of
    kept work matrices: the sequence on the live caches against every call as the first call of fresh ones (under the
    tolerance in force at that point of the sequence)."""
    from pycwt_amd import autograd, wavelet
    monkeypatch.setattr(autograd, "_engines", {})

    def forget():
        pycwt_amd.release_scratch()
        for p in wavelet._plans.values():
            p.close()
        for eng in autograd._engines.values():
            eng.plan.close()
        wavelet._plans.clear()
        autograd._engines.clear()
    ops = _shim_ops()
    try:
        fresh = []
        for name, op in ops:
            if name in SETTINGS:
                fresh.append(op() and None)
                continue
            forget()
            fresh.append(_arrays(op()))
        assert wavelet._tolerance is None            # (the sequence restores what it changes)
        forget()
        for (name, op), want in zip(ops, fresh):
            got = op()
            if name in SETTINGS:
                continue
            got = _arrays(got)
            assert len(got) == len(want), name
            for k, (a, b) in enumerate(zip(got, want)):
                assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (name, "output %d" % k)
        assert len(autograd._engines) == 1 and len(wavelet._plans) >= 2
    finally:
        pycwt_amd.set_tolerance(None)
        forget()
