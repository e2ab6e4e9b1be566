"""Call sequences on one live plan against fresh plans (plan_sequence_common.py: the catalogue, the two judgements, the sequences)
on a real MI355X: the sequences of tests/test_plan_sequences_emulated.py through the built library at nfft = 2^15, (a) and (b) also
at nfft = 2^18 with the production gates (default options; there (a) runs in PARTS thirds of an entry point's variations and the
walk of (b) in SEGMENTS consecutive pieces that share their end calls, so that a case stays at a few seconds with outputs of 70 MB:
every variation and every ordered pair is still there, asserted), and what only the device can show:

  streams        three torch streams; (b) with the plan moved to the next stream before every third call, (c) with the stream
                 changed between the call that uploads a derived copy and the call that evicts its slot: the bits of the default
                 stream.  At 2^18 the first long call on each new stream runs the queue probe, which may replace side streams
  back to back   (c): every input uploaded first, then the calls with no host synchronisation but the ABI's own, the outputs --
                 distinct buffers -- downloaded at the end: the events of a slot's previous copies are pending when it is rebuilt

No graph capture.  The fresh plans' results are memoised per (length, precision) for the whole module.
"""
import pytest

import plan_sequence_common as ps
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PRECS = [64, 32]
LOGNS = [ps.LOGN, 18]             # of the eviction sequences with a stream change
_runners = {}
_streams = []


def runner(lib, prec, logn=ps.LOGN):
    if not _streams:
        _streams.extend(torch.cuda.Stream() for _ in range(3))
    if (logn, prec) not in _runners:
        _runners[logn, prec] = ps.Runner(lib, 1 << logn, prec, TOL, options=ps.OPTS if logn == ps.LOGN else None,
                                         streams=[s.cuda_stream for s in _streams])
    return _runners[logn, prec]


def with_streams(steps, every=3):
    """the steps with the plan moved to the next of the three streams before every `every`-th call"""
    out, calls = [], 0
    for s in steps:
        if isinstance(s, ps.Call):
            if calls and calls % every == 0:
                out.append(ps.SetStream((calls // every) % 3))
            calls += 1
        out.append(s)
    return out


@pytest.mark.parametrize("prec", PRECS)
def test_the_grids_hold_every_form_on_the_device(hip_library, prec):
    a, e = ps.base_split(hip_library, 1 << ps.LOGN, prec), ps.base_split(hip_library, 1 << ps.LOGN, prec, name="E")
    assert all(a[f] > 0 for f in ("narrow", "ols", "aols", "poly")), a
    assert e["two_pass"] > 0, e


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("entry", ps.NAMES)
def test_a_one_argument_changes_on_the_device(hip_library, entry, prec):
    runner(hip_library, prec).run(ps.seq_one_argument(entry), "(a) " + entry)


PARTS = 3                 # of (a) at 2^18: outputs of 70 MB and their references, a few seconds per case
SEGMENTS = 6              # of the walk of (b) at 2^18


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("entry", ps.NAMES)
def test_a_one_argument_changes_under_the_production_gates(hip_library, entry, part, prec):
    """nfft = 2^18, default options; the variations of an entry point in PARTS interleaved thirds, each around the base call"""
    runner(hip_library, prec, 18).run(ps.seq_one_argument(entry, (part, PARTS)), "(a) %s, part %d" % (entry, part))


@pytest.mark.parametrize("prec", PRECS)
def test_b_all_ordered_pairs_on_the_device(hip_library, prec):
    made = runner(hip_library, prec).run(ps.seq_pairs(), "(b)")
    assert made == len(ps.POW2_NAMES) ** 2 + 1


@pytest.mark.parametrize("prec", PRECS)
def test_b_all_ordered_pairs_across_three_streams(hip_library, prec):
    runner(hip_library, prec).run(with_streams(ps.seq_pairs()), "(b) on three streams")


def test_the_segments_of_the_walk_hold_every_ordered_pair():
    walk = ps.seq_pairs()
    pieces = ps.segments(walk, SEGMENTS)
    assert set().union(*(ps.pairs_of([c.entry for c in p]) for p in pieces)) == {(a, b) for a in ps.POW2_NAMES for b in ps.POW2_NAMES}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("streams", [False, True], ids=["one-stream", "three-streams"])
@pytest.mark.parametrize("segment", range(SEGMENTS))
def test_b_all_ordered_pairs_under_the_production_gates(hip_library, segment, streams, prec):
    """nfft = 2^18, default options: the walk in SEGMENTS consecutive pieces that share their end calls (every ordered pair is in
    one of them), each on a live plan of its own; with the plan moved to the next of three streams before every third call, the
    first long call on each new stream runs the queue probe"""
    steps = ps.segments(ps.seq_pairs(), SEGMENTS)[segment]
    runner(hip_library, prec, 18).run(with_streams(steps) if streams else steps, "(b) segment %d" % segment)


@pytest.mark.parametrize("prec", PRECS)
def test_b_bluestein_between_power_of_two_calls_on_the_device(hip_library, prec):
    steps = ps.seq_pairs(ps.BLUESTEIN_MIX)
    steps += [ps.Call("bluestein", n0="small"), ps.Call("transform"), ps.Call("bluestein"), ps.Call("bluestein", n0="small")]
    runner(hip_library, prec).run(steps, "(b) bluestein")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("derived,other", ps.EVICTION_PAIRS)
def test_c_eviction_with_derived_copies_pending_on_the_device(hip_library, derived, other, prec):
    for k, steps in enumerate(ps.seq_eviction(derived, other)):
        runner(hip_library, prec).run(steps, "(c) %s / %s, sequence %d" % (derived, other, k), back_to_back=True)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("logn", LOGNS)
def test_c_eviction_with_the_stream_changed_before_the_slot_is_taken(hip_library, logn, prec):
    """the derived copy is uploaded on one stream, its slot evicted and rebuilt on the next, the copy made again on the third"""
    for derived, other in ps.EVICTION_PAIRS[:len(ps.EVICTION_PAIRS) if logn == ps.LOGN else 1]:
        first, second = ps.seq_eviction(derived, other)
        first = first[:2] + [ps.SetStream(1)] + first[2:6] + [ps.SetStream(2)] + first[6:]
        second = with_streams(second, every=2)
        for k, steps in enumerate((first, second)):
            runner(hip_library, prec, logn).run(steps, "(c) %s / %s on three streams, sequence %d" % (derived, other, k), back_to_back=True)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("toggle", ps.TOGGLES)
def test_d_invalidation_on_the_device(hip_library, toggle, prec):
    runner(hip_library, prec).run(ps.seq_invalidation(toggle, prec), "(d) " + toggle)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("entry", list(ps.SCRATCH))
def test_e_scratch_order_on_the_device(hip_library, entry, prec):
    for dim, up, down in ps.seq_scratch(entry):
        runner(hip_library, prec).run(up, "(e) %s, %s: small-large-small" % (entry, dim))
        runner(hip_library, prec).run(down, "(e) %s, %s: large-small-large" % (entry, dim))


@pytest.mark.parametrize("prec", PRECS)
def test_f_refused_calls_leave_no_trace_on_the_device(hip_library, prec):
    runner(hip_library, prec).run(ps.seq_refusals(), "(f)")


@pytest.mark.parametrize("prec", PRECS)
def test_f_refusal_that_has_taken_a_slot_on_the_device(hip_library, prec):
    runner(hip_library, prec).run(ps.seq_refusal_after_lookup(), "(f) a scale of 0")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("seed", ps.SEEDS)
def test_g_seeded_walks_on_the_device(hip_library, seed, prec):
    runner(hip_library, prec).run(ps.seq_walk(seed, prec), "(g) seed %d" % seed)
