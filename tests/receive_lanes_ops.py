"""The operation sequences of the receive-side lane stress (tests/test_receive_lanes_gpu.py), generated without a device so
that tests/test_receive_lanes_cpu.py can hold every seed the GPU test uses to its coverage conditions.

One seeded sequence mixes four kinds of operation on ONE context (Mode II, at most MAX_FRAMES frames per call):

  call     a chain call of 1 ... 8 frames on the context's own stream (it rotates over the lanes), from a pool of coded bits
           or -- `eti` -- from a pool of ETI frames through the front-end (dabgpu_frontend_process_dev on the context's own
           stream into one scratch buffer of coded bits, then the chain call), with or without FIRFilter, complexf or s16,
           into one of RING IQ buffers
  receive  one of the thirteen receive-side `_dev` entries with stream == NULL, on the most recent suitable buffer: a chain
           output that may still be in flight on lane 1 or 2, or the output of an earlier receive operation.  Every receive
           operation writes a tensor of its OWN (`tensors`), never the IQ ring.
  set      set_channel / channel_reset / decode_reset (with the decoders' lead-in fed again) / set_tii between calls
  fetch    a result getter: a host wait on the context's own stream

THE REUSE RULE.  The IQ ring has fewer buffers than a sequence has chain calls, so chain calls overwrite captures that queued
receive work reads -- on purpose.  The sequence stays inside the contract of include/dabgpu.h ("batches in flight"): two
lane calls are never ordered against each other, so
    a chain call is given an IQ buffer again only if a NULL-stream receive operation was queued after that buffer's last
    writer.
That receive operation runs behind every lane (so behind the last writer) and the new chain call starts behind it.  A chain
call that finds no such buffer is dropped.  Plan.check_reuse_rule() verifies the rule on the finished sequence, independently
of the code that chose the buffers.

Data flow: channel: chain output -> rx; sync then sync_extract: capture (chain output or rx of three frames or more) ->
frames; demod / demod_soft: whole frames (chain output, rx, extracted frames) -> bits / int8 metrics, `early` by the rule of
tests/demod_cases.py ((45 - 1) behind FIRFilter, else 0; CP / 2 behind the synchroniser, as the header advises); decode /
decode_soft: bits / metrics -> ETI images; tii_scan and cir on whole frames; spectrum and dpd_measure accumulate; the three
dpd entries take tx = a chain output and rx = the channel's complexf output of that very content.

A receive operation whose input does not exist yet gives way to the entry that makes it (a dpd entry without a live tx / rx
pair to channel, sync_extract without a synchronised capture to sync, decode* without bits or metrics to demod*), and a
chain call prefers the buffers whose content has been read, sparing the tx of the newest pair and a capture that has been
synchronised but not extracted yet.

Nothing here is tuned on a device: the weights below were chosen on the CPU until every seed met the conditions of
tests/test_receive_lanes_cpu.py.
"""
import numpy as np

MODE = 2                           # the smallest mode with TII
GEOM = dict(tf_samples=49152, tf_input_bytes=7200, null_size=664, sym_size=638, spacing=512)     # Mode II (asserted on the device)
CP = GEOM["sym_size"] - GEOM["spacing"]
MAX_FRAMES = 8
RING = 4                           # IQ buffers the chain calls write
POOL_FRAMES = 16                   # coded-bit frames the calls draw from
ETI_POOL = 24                      # ETI frames the front-end calls draw from (Mode II: one per transmission frame)
SEEDS = (20, 22, 32)               # chosen on the CPU: tests/test_receive_lanes_cpu.py holds for them at DEFAULT_OPS
DEFAULT_OPS = 330
GAIN, FIR = 1, 2
ENTRIES = ("channel", "sync", "sync_extract", "demod", "demod_soft", "decode", "decode_soft", "tii_scan", "cir", "spectrum",
           "dpd_xspectrum", "dpd_align", "dpd_measure")
DPD_PEAK, DPD_BINS = 40000.0, 64
# Sizes from the mutation protocol (profiles/receive_lane_stress_mutations.txt): transmission frames per call of the directed
# tests, and transmission frames per generated frame of the stress (a call of f frames here runs f x STRESS_UNIT)
DIRECTED_FRAMES = 256
STRESS_UNIT = 1
# The decoders return zeros for the first fifteen frames of a stream (include/dabgpu.h).  So that every output of the sequence
# is payload, both decoders take DECODER_PRIME calls of MAX_FRAMES frames of zeros before the sequence starts, and again as
# part of every decode_reset operation (queued like the rest).
DECODER_PRIME = 2

# Weights of the four kinds, by what the operation before was: calls and receive operations alternate more often than not,
# so that a receive operation finds a chain output in flight and a chain call finds a buffer that has been read.  Among the
# receive operations an entry's weight falls by a factor of four for every occurrence it is ahead of the rarest entry, which
# keeps the thirteen level: dabgpu_dpd_align_dev solves two alignments on the host, 10 ms a call, so the sequence holds no
# more of any entry than the coverage conditions ask for.
KIND_WEIGHTS = {"call": (("call", 0.32), ("receive", 0.56), ("set", 0.05), ("fetch", 0.07)),
                "receive": (("call", 0.62), ("receive", 0.26), ("set", 0.05), ("fetch", 0.07))}
ENTRY_WEIGHTS = dict.fromkeys(ENTRIES, 1.0)


def seed_of(seed):
    return 9100 + int(seed)


class Plan:
    """ops: one dict per drawn operation (kind "drop" where nothing suitable existed); tensors: (dtype name, elements) of every
    tensor a receive operation writes, in order of creation.  A buffer is named ("iq", ring index) or ("t", tensor index)."""

    def __init__(self):
        self.ops, self.tensors = [], []

    # ---- the figures of tests/test_receive_lanes_cpu.py, recomputed from `ops` alone --------------------------------------
    def entry_counts(self):
        c = dict.fromkeys(ENTRIES, 0)
        for op in self.ops:
            if op["kind"] == "receive":
                c[op["entry"]] += 1
        return c

    def _walk(self):
        """-> per receive operation whether it reads an IQ buffer whose last writer was a chain call with nothing on the
        context's own stream (and no setter that waits for the context) in between; per chain call whether the content it
        overwrites was read by a receive operation; and the reuse rule's violations"""
        writer = [None] * RING            # tick of the chain call that wrote the buffer last
        own = -1                          # tick of the most recent work on the context's own stream
        recv_after = [False] * RING
        was_read = [False] * RING
        raw, war, bad = [], [], []
        tick = 0
        for i, op in enumerate(self.ops):
            k = op["kind"]
            if k == "call":
                b = op["ring"]
                if op["eti"]:             # the front-end runs on the context's own stream, in front of its chain call
                    own = tick
                    tick += 1
                if writer[b] is not None and not recv_after[b]:
                    bad.append(i)
                war.append(writer[b] is not None and was_read[b])
                writer[b], recv_after[b], was_read[b] = tick, False, False
            elif k == "receive":
                hit = False
                for name, idx in op["reads"]:
                    if name == "iq":
                        assert writer[idx] is not None, i
                        hit = hit or own < writer[idx]
                        was_read[idx] = True
                raw.append(hit)
                own = tick
                recv_after = [w is not None for w in writer]
            elif k == "set" and op["what"] in ("decode_reset", "set_tii"):
                own = tick                # decode_reset waits for the context; a TII change may drain the lanes at the next call
            tick += 1
        return raw, war, bad

    def check_reuse_rule(self):
        """the indices of the chain calls that break the reuse rule (none, if the generator is right)"""
        return self._walk()[2]

    def coverage(self):
        raw, war, _ = self._walk()
        kinds = [op["kind"] for op in self.ops]
        calls = [op for op in self.ops if op["kind"] == "call"]
        return dict(ops=len(self.ops), calls=len(calls), receives=len(raw), raw_share=sum(raw) / max(len(raw), 1),
                    war_share=sum(war) / max(len(war), 1), dropped_share=kinds.count("drop") / max(len(kinds), 1),
                    fetch_share=kinds.count("fetch") / max(len(kinds), 1),
                    capture_share=sum(op["frames"] >= 3 for op in calls) / max(len(calls), 1),
                    eti_calls=sum(op["eti"] for op in calls), entries=self.entry_counts())


def _settings(rs):
    k = rs.randint(6)
    if k <= 1:
        paths = [(0, 1.0 + 0.0j, 0.0)]
        for _ in range(int(rs.randint(0, 3))):
            gain = float(rs.uniform(0.1, 0.5)) * np.exp(2j * np.pi * float(rs.rand()))
            paths.append((int(rs.randint(1, 300)), complex(np.complex64(gain)), float(rs.choice([0.0, 5.0, -12.5]))))
        return dict(kind="set", what="set_channel", paths=paths, sigma=float(rs.choice([0.0, 20.0, 100.0])),
                    seed=int(rs.randint(1, 2 ** 31 - 1)))
    if k == 2:
        return dict(kind="set", what="channel_reset", position=int(rs.choice([0, 12345, 2 ** 33 + 7])))
    if k == 3:
        return dict(kind="set", what="decode_reset")
    return dict(kind="set", what="set_tii", on=bool(rs.randint(2)), comb=int(rs.randint(1, 24)), pattern=int(rs.randint(0, 70)))


def generate(seed, n_ops=DEFAULT_OPS):
    rs = np.random.RandomState(seed_of(seed))
    tf, per = GEOM["tf_samples"], GEOM["tf_input_bytes"]
    plan = Plan()
    ring = [None] * RING                  # dict(version, frames, fmt, early, tick, recv_after, was_read)
    sources = []                          # whole-frame buffers the receive entries read: dict(buf, kind, frames, fmt, early, tick, token)
    bits, softs = [], []                  # dict(buf, frames)
    pairs = []                            # dict(tx ring index, its version, rx tensor, samples)
    synced = None                         # the capture of the most recent sync: its source dict
    done = set()                          # which results exist: what a fetch may ask for
    demod_frames, decoded = 0, {}
    force_cf = extracted = False
    tick = 0
    entries, ew = list(ENTRIES), np.array([ENTRY_WEIGHTS[e] for e in ENTRIES])
    count = dict.fromkeys(ENTRIES, 0)
    before = "receive"

    def live(s):
        return s["token"] is None or ring[s["token"][0]]["version"] == s["token"][1]

    def newest(pred):
        c = [s for s in sources if live(s) and pred(s)]
        return max(c, key=lambda s: s["tick"]) if c else None

    def tensor(dtype, n):
        plan.tensors.append((dtype, int(n)))
        return ("t", len(plan.tensors) - 1)

    def meta(s):
        return dict(buf=s["buf"], frames=s["frames"], fmt=s["fmt"])

    for _ in range(n_ops):
        tick += 1
        kinds, kw = [k for k, _ in KIND_WEIGHTS[before]], np.array([w for _, w in KIND_WEIGHTS[before]])
        kind = kinds[int(rs.choice(len(kinds), p=kw / kw.sum()))]
        op = None
        if kind == "call":
            frames = int(rs.choice([1, 1, 2, 2, 3, 4, 5, 8]))
            stages = int(rs.choice([GAIN, GAIN | FIR, GAIN | FIR]))
            fmt = "s16" if rs.rand() < 0.3 else "cf"
            eti = bool(rs.rand() < 0.25)
            at = int(rs.randint(0, (ETI_POOL if eti else POOL_FRAMES) - frames + 1))
            ok = [b for b in range(RING) if ring[b] is None or ring[b]["recv_after"]]
            if ok:
                # the content a receive operation has read first (the write-after-read case), the oldest of it first
                # (... the tx of the newest tx / rx pair last, so that a dpd entry still finds it,
                # and the capture the synchroniser saw last, until it has been extracted)
                keep = {pairs[-1]["tx"]} if pairs and ring[pairs[-1]["tx"]]["version"] == pairs[-1]["version"] else set()
                if synced is not None and synced["token"] is not None and live(synced) and not extracted:
                    keep.add(synced["token"][0])
                b = min(ok, key=lambda b: (ring[b] is not None, b in keep, ring[b] is not None and not ring[b]["was_read"],
                                           ring[b]["tick"] if ring[b] else 0))
                version = ring[b]["version"] + 1 if ring[b] else 1
                early = 44 if stages & FIR else 0
                ring[b] = dict(version=version, frames=frames, fmt=fmt, early=early, tick=tick, recv_after=False, was_read=False)
                sources.append(dict(buf=("iq", b), kind="chain", frames=frames, fmt=fmt, early=early, tick=tick, token=(b, version)))
                sources = [s for s in sources if live(s)][-64:]
                op = dict(kind="call", ring=b, frames=frames, stages=stages, fmt=fmt, eti=eti, at=at)
        elif kind == "set":
            op = _settings(rs)
        elif kind == "fetch":
            have = sorted(done)
            if have:
                what = have[int(rs.randint(len(have)))]
                op = dict(kind="fetch", what=what)
                if what == "monitor":
                    op["frame"] = int(rs.randint(demod_frames))
                elif what.startswith("decode"):
                    op["frame"] = int(rs.randint(decoded[what]))
        else:
            have = np.array([count[e] for e in entries])
            w = ew * 0.25 ** (have - have.min())
            e = entries[int(rs.choice(len(entries), p=w / w.sum()))]
            reads, args, out = [], {}, None
            # an entry whose input does not exist yet gives way to the entry that makes it (one step: no chain of them)
            if e.startswith("dpd_") and not [p for p in pairs if ring[p["tx"]]["version"] == p["version"]]:
                e, force_cf = "channel", True
            elif e == "sync_extract" and not (synced is not None and live(synced)):
                e = "sync"
            elif e == "decode" and not bits:
                e = "demod"
            elif e == "decode_soft" and not softs:
                e = "demod_soft"
            else:
                force_cf = False
            if e == "channel":
                s = newest(lambda s: s["kind"] == "chain")
                if s:
                    ofmt = "s16" if rs.rand() < 0.15 and not force_cf else "cf"
                    out = tensor("complex64" if ofmt == "cf" else "int16", s["frames"] * tf * (1 if ofmt == "cf" else 2))
                    reads, args = [s["buf"]], dict(src=meta(s))
                    sources.append(dict(buf=out, kind="rx", frames=s["frames"], fmt=ofmt, early=s["early"], tick=tick, token=None))
                    if ofmt == "cf":
                        pairs.append(dict(tx=s["token"][0], version=s["token"][1], txmeta=meta(s), rx=out, samples=s["frames"] * tf))
            elif e == "sync":
                s = newest(lambda s: s["kind"] in ("chain", "rx") and s["frames"] >= 3)
                if s:
                    reads, args, synced, extracted = [s["buf"]], dict(src=meta(s), max_shift=int(rs.choice([31, 8]))), s, False
                    done.add("sync")
            elif e == "sync_extract":
                if synced is not None and live(synced):
                    s, extracted = synced, True
                    out = tensor("complex64", s["frames"] * tf)
                    reads, args = [s["buf"]], dict(src=meta(s))
                    sources.append(dict(buf=out, kind="frames", frames=s["frames"], fmt="cf", early=CP // 2, tick=tick, token=None))
            elif e in ("demod", "demod_soft"):
                s = newest(lambda s: True)
                if s:
                    reads, args = [s["buf"]], dict(src=meta(s), early=s["early"])
                    if e == "demod":
                        out = tensor("uint8", s["frames"] * per)
                        bits.append(dict(buf=out, frames=s["frames"]))
                    else:
                        args["bits"] = tensor("uint8", s["frames"] * per) if rs.rand() < 0.5 else None
                        out = tensor("int8", 8 * s["frames"] * per)
                        softs.append(dict(buf=out, frames=s["frames"]))
                    done.add("monitor")
                    demod_frames = s["frames"]
            elif e in ("decode", "decode_soft"):
                have = bits if e == "decode" else softs
                if have:
                    s = have[-1]
                    out = tensor("uint8", s["frames"] * 6144)
                    reads, args = [s["buf"]], dict(src=dict(buf=s["buf"], frames=s["frames"]))
                    done.add(e + "_stats")
                    decoded[e + "_stats"] = s["frames"]           # (Mode II: one ETI image per transmission frame)
            elif e == "tii_scan":
                s = newest(lambda s: s["frames"] >= 2)
                if s:
                    reads = [s["buf"]]
                    args = dict(src=meta(s), early=min(s["early"], GEOM["null_size"] - GEOM["spacing"]))
                    done.add("tii_scan")
            elif e == "cir":
                s = newest(lambda s: True)
                if s:
                    reads, args = [s["buf"]], dict(src=meta(s), early=s["early"], window=int(rs.randint(2)))
                    done.add("cir")
            elif e == "spectrum":
                s = newest(lambda s: True)
                if s:
                    reads, args = [s["buf"]], dict(src=meta(s))
                    done.add("spectrum")
            else:
                c = [p for p in pairs if ring[p["tx"]]["version"] == p["version"]]
                if c:
                    p = c[-1]
                    reads, args = [("iq", p["tx"]), p["rx"]], dict(tx=p["txmeta"], rx=p["rx"], samples=p["samples"])
                    if e == "dpd_xspectrum":
                        args["rx_offset"] = int(rs.choice([0, 3, -2]))
                        done.add("dpd_xspectrum")
                    elif e == "dpd_align":
                        done.add("dpd_xspectrum")
                    else:
                        args["alignment"] = None if rs.rand() < 0.5 else dict(lag=int(rs.randint(-3, 4)), tau=float(rs.choice([0.0, 0.25, -0.4])),
                                                                              gain=complex(1.0, 0.0))
                        done.add("dpd_stats")
            if reads:
                op = dict(kind="receive", entry=e, reads=reads, out=out, **args)
                count[e] += 1
                for b in range(RING):
                    if ring[b] is not None:
                        ring[b]["recv_after"] = True
                for name, idx in reads:
                    if name == "iq":
                        ring[idx]["was_read"] = True
                pairs = pairs[-16:]
        plan.ops.append(op if op is not None else dict(kind="drop", drawn=kind))
        if op is not None and op["kind"] in ("call", "receive"):
            before = op["kind"]
    return plan
