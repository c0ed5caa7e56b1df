"""The superframe reader's model (tests/superframe_model.py) -- the oracle of tests/test_superframe_gpu.py -- held to the reference's
Reed-Solomon code (lib/fec behind oracle.ref(), live where it was built, and from tests/golden/superframe_rs.json everywhere), to
the standard's Fire code and header table, and the greedy walk to hand-made record lists; the host-only shape check of the
library.  All integers."""
import numpy as np
import pytest

import oracle as O
from tests import superframe_cases as SC
from tests import superframe_model as SM

needs_ref = pytest.mark.skipif(not O.have_ref(), reason="the reference's library was not built here")


# --------------------------------------------------------------------------- 1. the model against the reference's code, live
@needs_ref
def test_parity_equals_the_references_encoder():
    fec, rs = SC.Libfec(), np.random.RandomState(11)
    for _ in range(200):
        data = bytes(rs.randint(0, 256, SM.K).astype(np.uint8))
        assert SM.rs_parity(data) == fec.parity(data)
    assert SM.rs_parity(bytes(SM.K)) == bytes(10) and SM.rs_decode(SM.rs_encode(bytes(range(SM.K)))) == (SM.rs_encode(bytes(range(SM.K))), 0)


@needs_ref
@pytest.mark.parametrize("n_err", [1, 2, 3, 4, 5])
def test_up_to_five_errors_are_corrected_as_the_reference_corrects_them(n_err):
    """2000 words per count; the first ones with errors on the edge positions 0, 63, 64, 109, 110, 119"""
    fec, rs = SC.Libfec(), np.random.RandomState(20 + n_err)
    for k in range(2000):
        must = SC.EDGES[k % 6:][:n_err] if k < 12 else ()
        word = SC.random_word(rs)
        bad = SC.corrupt(word, rs, n_err, must)
        after, ret, loc = fec.decode(bad)
        assert (after, ret) == (word, n_err) and min(loc) >= SM.PAD
        assert SM.rs_decode(bad) == (word, n_err), (bad.hex(), loc)


@needs_ref
def test_beyond_five_errors_the_model_refuses_what_the_reference_refuses_and_every_padding_root():
    """6 ... 12 errors.  Per word about 99.2 % are refused, 0.7 % have a root in the 135 padding positions (lib/fec corrects the rest
    of the locator and reports success; the model refuses and leaves the bytes alone) and 0.01 % are miscorrected to another
    codeword.  4000 words give about 28 padding cases (none: 6e-13); the search for miscorrections goes on with lib/fec alone
    (60 000 words: none with probability e^-6) and the model sees every one that is not refused."""
    fec, rs = SC.Libfec(), np.random.RandomState(612)
    seen = dict(refused=0, padding=0, miscorrected=0, corrected=0)
    for k in range(60000):
        word = SC.random_word(rs) if k < 4000 else word
        bad = SC.corrupt(word, rs, 6 + k % 7)
        after, ret, loc = fec.decode(bad)
        kind = SC.classify(ret, loc)
        if kind == "refused" and k >= 4000:
            seen[kind] += 1
            continue
        seen[SC.check_against_libfec(bad, after, ret, loc, word)] += 1
        if k >= 4000 and seen["miscorrected"] >= 2:
            break
    print("beyond t:", seen)
    assert seen["refused"] > 3900 and seen["padding"] >= 10 and seen["miscorrected"] >= 1 and seen["corrected"] == 0


# --------------------------------------------------------------------------- 2. the same from the fixture
def test_the_fixture_holds_every_class_and_the_model_agrees_with_it():
    entries = SC.golden()
    assert 150 <= len(entries) <= 250
    kinds = {}
    for e in entries:
        word, bad, after = (bytes.fromhex(e[k]) for k in ("word", "bad", "after"))
        assert SM.rs_decode(word) == (word, 0) and sum(a != b for a, b in zip(word, bad)) == e["n_err"]
        kind = SC.check_against_libfec(bad, after, e["ret"], e["loc"], word)
        kinds[kind] = kinds.get(kind, 0) + 1
        if e["n_err"] <= 5:
            assert kind == "corrected" and e["ret"] == e["n_err"] and after == word
    assert kinds["corrected"] >= 100 and kinds["refused"] >= 30 and kinds["padding"] >= 20 and kinds["miscorrected"] >= 3
    hit = {p for e in entries if e["n_err"] <= 5 for p in range(SM.N) if e["word"][2 * p:2 * p + 2] != e["bad"][2 * p:2 * p + 2]}
    assert set(SC.EDGES) <= hit


# --------------------------------------------------------------------------- 3. Fire code
def clmul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        b >>= 1
    return r


def test_fire_code_polynomial_zero_header_and_single_bit_changes():
    assert clmul((1 << 11) | 1, 0b101111) == 0x1782F               # (x^11 + 1)(x^5 + x^3 + x^2 + x + 1)
    assert SM.fire_crc(b"\x00\x01") == 0x782F                      # a single one, shifted out: the polynomial's low 16 bits
    # the division, bit by bit: nine bytes times x^16, remainder by the 17-bit polynomial
    rs = np.random.RandomState(3)
    for _ in range(20):
        msg = bytes(rs.randint(0, 256, 9).astype(np.uint8))
        rem = int.from_bytes(msg, "big") << 16
        for bit in range(rem.bit_length() - 1, 15, -1):
            if rem >> bit & 1:
                rem ^= 0x1782F << (bit - 16)
        assert SM.fire_crc(msg) == rem
    s = 2
    rec, _ = SM.candidate(bytes(SM.N * s), s)
    assert rec["flags"] & SM.FIRE_OK and rec["flags"] & SM.ZERO and not SM.accepted(rec) and rec["au_ok"] == 0
    sf, _ = SM.build_superframe(s, np.random.RandomState(1))
    rec, out = SM.candidate(sf, s)
    assert SM.accepted(rec) and rec["au_ok"] == (1 << rec["num_aus"]) - 1 and rec["rs_corrected"] == 0
    for bit in range(88):                                         # bytes 0 ... 10; the words re-encoded so that RS does not undo it
        data = bytearray(out)
        data[bit // 8] ^= 0x80 >> bit % 8
        rec, _ = SM.candidate(SM.rs_protect(bytes(data), s), s)
        assert not rec["flags"] & SM.FIRE_OK and rec["au_ok"] == 0 and not SM.accepted(rec), bit


# --------------------------------------------------------------------------- 4. header
@pytest.mark.parametrize("dac_rate,sbr_flag,num,first", [(0, 1, 2, 5), (1, 1, 3, 6), (0, 0, 4, 8), (1, 0, 6, 11)])
def test_header_rows(dac_rate, sbr_flag, num, first):
    s = 3
    sf, aus = SM.build_superframe(s, np.random.RandomState(5), dac_rate=dac_rate, sbr_flag=sbr_flag, channel_mode=1, ps_flag=sbr_flag, surround=2)
    rec, out = SM.candidate(sf, s)
    assert SM.accepted(rec) and (rec["num_aus"], rec["au_start"][0], rec["au_start"][num]) == (num, first, 110 * s)
    assert rec["au_start"][num + 1:] == [0] * (6 - num) and rec["au_ok"] == (1 << num) - 1
    assert (rec["rfa"], rec["dac_rate"], rec["sbr_flag"], rec["aac_channel_mode"], rec["ps_flag"], rec["mpeg_surround_config"]) == \
        (0, dac_rate, sbr_flag, 1, sbr_flag, 2)
    res = SM.walk([rec])
    assert SM.slice_aus(out, res, [rec], s) == (aus, [True] * num)
    assert SM.unpack_record(SM.pack_record(rec)) == rec


def with_starts(s, starts):
    """a superframe with dac_rate 1, sbr 1 (three AUs from byte 6) whose two start fields are `starts`; Fire code and RS in order"""
    data = bytearray(110 * s)
    data[2] = 0x60
    data[3:6] = (starts[0] << 12 | starts[1]).to_bytes(3, "big")
    c = SM.fire_crc(data[2:11])
    data[0], data[1] = c >> 8, c & 0xFF
    return SM.candidate(SM.rs_protect(bytes(data), s), s)[0]


def test_header_validity():
    s = 2
    ok = with_starts(s, (9, 12))
    assert ok["flags"] & SM.HEADER_VALID and ok["flags"] & SM.FIRE_OK and ok["au_start"][:4] == [6, 9, 12, 220]
    for starts in [(100, 50), (50, 50), (8, 100), (100, 218), (100, 221), (100, 4095)]:   # descending, equal, short first / last AU, beyond
        r = with_starts(s, starts)
        assert not r["flags"] & SM.HEADER_VALID and r["flags"] & SM.FIRE_OK and not SM.accepted(r) and r["au_ok"] == 0, starts
    assert with_starts(s, (100, 217))["flags"] & SM.HEADER_VALID


# --------------------------------------------------------------------------- 5. the walk
GOOD = dict(flags=SM.FIRE_OK | SM.HEADER_VALID, num_aus=3, au_ok=7, rs_corrected=2, rs_failed=0, rs_max=2)
NOISE = dict(flags=0, num_aus=4, au_ok=0, rs_corrected=0, rs_failed=3, rs_max=0)
LEADIN = dict(flags=SM.FIRE_OK | SM.ZERO | SM.HEADER_VALID, num_aus=4, au_ok=0, rs_corrected=0, rs_failed=0, rs_max=0)


@pytest.mark.parametrize("phase", range(5))
def test_walk_finds_every_phase(phase):
    recs = [GOOD if f % 5 == phase else NOISE for f in range(23)]
    res = SM.walk(recs)
    want = list(range(phase, 23, 5))
    assert res["accepted"] == want and res["first"] == phase and res["superframes"] == len(want) and res["phase_changes"] == 0
    assert (res["aus"], res["aus_ok"], res["aus_bad"], res["rs_corrected"], res["rs_failed"], res["rs_max"]) == \
        (3 * len(want), 3 * len(want), 0, 2 * len(want), 0, 2)


def test_walk_over_a_lost_superframe_a_false_candidate_and_the_lead_in():
    recs = [GOOD if f % 5 == 1 else NOISE for f in range(30)]
    recs[11] = dict(NOISE)                                         # lost: the walk goes on candidate by candidate
    res = SM.walk(recs)
    assert res["accepted"] == [1, 6, 16, 21, 26] and res["phase_changes"] == 0 and res["candidates"] == 30
    recs = [GOOD if f % 5 == 1 else NOISE for f in range(30)]
    false = dict(GOOD, au_ok=1, rs_failed=1, flags=GOOD["flags"] | SM.RS_FAILED)
    recs[8] = false                                                # a false one between 6 and 11: the walk steps over it
    res = SM.walk(recs)
    assert res["accepted"] == [1, 6, 11, 16, 21, 26] and res["phase_changes"] == 0 and res["aus_bad"] == 0
    recs[11], recs[13] = NOISE, false                              # behind a lost one it is taken, and costs the good one at 16
    res = SM.walk(recs)
    assert res["accepted"] == [1, 6, 13, 21, 26] and res["phase_changes"] == 2
    assert (res["aus_bad"], res["aus_ok"], res["rs_failed"]) == (2, 13, 1)
    recs = [LEADIN] * 15 + [GOOD if f % 5 == 2 else NOISE for f in range(15)]
    res = SM.walk(recs)
    assert res["accepted"] == [17, 22, 27] and res["first"] == 17
    res = SM.walk([LEADIN] * 12)
    assert res["superframes"] == 0 and res["first"] == -1 and res["accepted"] == [] and res["candidates"] == 12


# --------------------------------------------------------------------------- 6. the library's shape check
def test_superframe_check_refusals(pkg):
    pkg.build()
    pkg.superframe_check(5, 0, 24)
    pkg.superframe_check(1 << 22, 6144 - 576, 576)
    pkg.superframe_check(9, 12 + 4 + 96, 96)
    for args, why in [((4, 0, 24), "n_images must lie in 5 ... 2\\^22"), (((1 << 22) + 1, 0, 24), "n_images must lie in"),
                      ((5, 0, 0), "framesize must be 24 s"), ((5, 0, 100), "framesize must be 24 s"), ((5, 0, 600), "framesize must be 24 s"),
                      ((5, 6, 24), "offset must be a multiple of 4"), ((5, 6144 - 20, 24), "exceeds the 6144-byte image"),
                      ((5, 1 << 40, 24), "exceeds the 6144-byte image")]:
        with pytest.raises(pkg.DabGpuError, match=why):
            pkg.superframe_check(*args)
