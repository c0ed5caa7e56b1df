"""The operation sequences of tests/test_receive_lanes_gpu.py, checked without a device: for every seed and at the operation
count the GPU test runs by default, the generator (tests/receive_lanes_ops.py) keeps its reuse rule and covers what the
stress is there for.  The seeds and weights were chosen here, on the CPU; nothing is tuned on the device."""
import pytest

from tests import receive_lanes_ops as G


@pytest.fixture(scope="module")
def plans():
    return {seed: G.generate(seed, G.DEFAULT_OPS) for seed in G.SEEDS}


def test_the_gpu_test_uses_three_seeds_and_the_sequences_repeat():
    assert len(set(G.SEEDS)) == 3
    a, b = G.generate(G.SEEDS[0], 120), G.generate(G.SEEDS[0], 120)
    assert a.ops == b.ops and a.tensors == b.tensors
    assert G.generate(G.SEEDS[1], 120).ops != a.ops


@pytest.mark.parametrize("seed", G.SEEDS)
def test_a_chain_call_reuses_a_buffer_only_behind_a_receive_operation(plans, seed):
    """The reuse rule of the module docstring, recomputed from the finished sequence: whenever a chain call writes an IQ
    buffer that holds an earlier call's output, a NULL-stream receive operation was queued after that earlier call.  And the
    ring really is reused: far more calls than buffers."""
    plan = plans[seed]
    assert plan.check_reuse_rule() == []
    calls = [op for op in plan.ops if op["kind"] == "call"]
    assert len(calls) > 10 * G.RING and {op["ring"] for op in calls} == set(range(G.RING))
    # the check itself has teeth: a sequence with its receive operations taken out breaks the rule
    stripped = G.Plan()
    stripped.ops = [op for op in plan.ops if op["kind"] != "receive"]
    assert stripped.check_reuse_rule()


@pytest.mark.parametrize("seed", G.SEEDS)
def test_every_receive_operation_reads_what_exists_in_the_shape_its_entry_takes(plans, seed):
    """Inputs are buffers that have been written, in the sizes the entries accept (include/dabgpu.h): three frames or more for
    the synchroniser, two or more for the TII analyser, at most max_frames everywhere, `early` inside the cyclic prefix (the
    null symbol's slack for tii_scan), an extraction only of the capture the most recent sync was given."""
    plan = plans[seed]
    written, synced = set(), None
    for op in plan.ops:
        if op["kind"] == "call":
            assert 1 <= op["frames"] <= G.MAX_FRAMES and op["stages"] in (G.GAIN, G.GAIN | G.FIR) and op["fmt"] in ("cf", "s16")
            assert 0 <= op["at"] and op["at"] + op["frames"] <= (G.ETI_POOL if op["eti"] else G.POOL_FRAMES)
            written.add(("iq", op["ring"]))
        elif op["kind"] == "receive":
            assert all(tuple(r) in written for r in op["reads"]), op
            e = op["entry"]
            if e.startswith("dpd_"):
                assert op["tx"]["frames"] * G.GEOM["tf_samples"] == op["samples"] >= 2048
            else:
                n = op["src"]["frames"]
                assert 1 <= n <= G.MAX_FRAMES
                if e in ("sync", "sync_extract"):
                    assert n >= 3
                if e == "sync":
                    synced = op["src"]
                if e == "sync_extract":
                    assert op["src"] == synced
                if e == "tii_scan":
                    assert n >= 2 and 0 <= op["early"] <= G.GEOM["null_size"] - G.GEOM["spacing"]
                if e in ("demod", "demod_soft", "cir"):
                    assert 0 <= op["early"] <= G.CP
            if op["out"] is not None:
                written.add(tuple(op["out"]))
            if op.get("bits") is not None:
                written.add(tuple(op["bits"]))
        elif op["kind"] == "fetch":
            assert op["what"] in ("sync", "tii_scan", "cir", "monitor", "spectrum", "dpd_xspectrum", "dpd_stats", "decode_stats",
                                  "decode_soft_stats")
    assert len(plan.tensors) == len([t for t in written if t[0] == "t"])


@pytest.mark.parametrize("seed", G.SEEDS)
def test_the_sequences_cover_what_the_stress_is_for(plans, seed):
    c = plans[seed].coverage()
    print(c)
    assert c["ops"] == G.DEFAULT_OPS
    # each of the thirteen entries at least ten times
    assert set(c["entries"]) == set(G.ENTRIES) and len(G.ENTRIES) == 13
    assert min(c["entries"].values()) >= 10, c["entries"]
    # read-after-write across lanes: the reader's buffer was last written by a chain call, nothing on the own stream since
    assert c["raw_share"] >= 0.30
    # write-after-read: the chain call overwrites content a receive operation has read
    assert c["war_share"] >= 0.20
    assert c["dropped_share"] <= 0.05
    # every fetch is a host wait on the context's own stream: too many would serialise the run
    assert c["fetch_share"] <= 0.10
    # a third of the calls or more can serve the synchroniser as a capture; some calls come through the front-end
    assert c["capture_share"] >= 1.0 / 3.0 and c["eti_calls"] >= 10
    # every kind of setting and of result occurs
    assert {op["what"] for op in plans[seed].ops if op["kind"] == "set"} == {"set_channel", "channel_reset", "decode_reset", "set_tii"}
    assert {op["what"] for op in plans[seed].ops if op["kind"] == "fetch"} >= {"sync", "tii_scan", "cir", "monitor", "spectrum",
                                                                             "dpd_xspectrum", "dpd_stats"}
