"""The host half of the FIC reader (include/dabgpu.h, "the FIC reader"; odr-dabmod_amd/csrc/api_fic.hip), without a device: the
ETI header made from a result, the short-form table and the derived fields, the bootstrap frame, the refusals -- against the
plain-Python model (tests/fic_model.py) and against dabgpu_frontend_describe of the frames the layouts came from.  All
integers, every comparison is equality."""
import copy

import numpy as np
import pytest

from tests import decode_cases as K
from tests import fic_cases as FC
from tests import fic_model as FM
from tests.golden.frontend_cases import ETI_CASES, PUNCTURE_CASES
from tests.golden.synth import synth_eti

ROUND_TRIP = {name: (ETI_CASES[name]["mode"], ETI_CASES[name]["kw"]) for name in ("cfg1", "multi", "mode2", "mode3", "mode4")}
ROUND_TRIP["twelve"] = (1, dict(subchannels=K.TWELVE))


def model_result(eti, mode):
    lay_off = 12 + 4 * (int(eti[0, 5]) & 0x7F)
    return FM.scan(FM.fibs_of(eti, lay_off, 128 if mode == 3 else 96))[1]


def one_subch(entry, **over):
    """the result of a scan that saw this one FIG 0/1 entry once"""
    res = FM.scan([FC.fib([FC.fig0_1([entry])])])[1]
    res["sub"][0].update(over)
    return res


def test_crc_of_the_standard_check_strings():
    assert FM.crc16(b"123456789") == 0xD64E and FM.crc16(bytes(30)) == 0xD5BA


@pytest.mark.parametrize("name", list(ROUND_TRIP))
def test_header_made_from_the_fic_describes_as_the_original_frame(pkg, name):
    """The layout's own FIC -> the model's result -> fic_make_header -> frontend_describe: every field equals the original's.
    (These cases number their sub-channels in STC order, so ascending SubChId is the same order.)"""
    mode, kw = ROUND_TRIP[name]
    eti = FC.with_fic(synth_eti(4, **kw), mode)
    res = model_result(eti, mode)
    assert res["n_subch"] == len(kw.get("subchannels", (0,))) and res["fibs_bad"] == 0 and res["fibs_ok"] == res["fibs"]
    assert all(s["changes"] == 0 and s["seen"] == 4 and s["supported"] for s in res["sub"])
    frame = pkg.fic_make_header(res, mode)
    assert bytes(frame) == FM.make_header(res, mode)
    assert pkg.Modulator.frontend_describe(frame) == pkg.Modulator.frontend_describe(eti[0])
    pkg.decode_check_layout(frame)


def test_all_64_short_form_rows_give_the_size_of_the_puncturing_profile(pkg):
    fe = K.cpu_front_end()
    assert [r[0] for r in FM.SHORT_TABLE] == sorted(r[0] for r in FM.SHORT_TABLE)
    for index in range(64):
        res = one_subch(FC.sub_short(9, 100, index))
        s = res["sub"][0]
        assert (s["bitrate"], s["level"], s["size_cu"]) == FM.SHORT_TABLE[index] and s["tpl"] == s["level"] - 1
        prof = fe.subchannel_profile(s["stl"], s["tpl"])
        assert prof is not None and prof[1] == s["size_cu"] and prof[2] == s["bitrate"], index
        lay = pkg.Modulator.frontend_describe(pkg.fic_make_header(res, 1))
        assert [(x["sad"], x["stl"], x["tpl"], x["cu"]) for x in lay["subchannels"]] == [(100, s["stl"], s["tpl"], s["size_cu"])]


def test_every_eep_puncture_case_round_trips_through_the_long_form(pkg):
    fe = K.cpu_front_end()
    cases = [(stl, tpl) for stl, tpl in PUNCTURE_CASES if tpl & 0x20 and fe.subchannel_profile(stl, tpl) is not None]
    assert len(cases) >= 10
    for stl, tpl in cases:
        entry = FC.entry_of(5, 40, stl, tpl)
        assert len(entry) == 4
        res = one_subch(entry)
        s = res["sub"][0]
        assert (s["stl"], s["tpl"], s["supported"], s["size_cu"]) == (stl, tpl, 1, fe.subchannel_profile(stl, tpl)[1]), (stl, tpl)
        lay = pkg.Modulator.frontend_describe(pkg.fic_make_header(res, 2))
        assert [(x["sad"], x["stl"], x["tpl"], x["cu"]) for x in lay["subchannels"]] == [(40, stl, tpl, s["size_cu"])]


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_bootstrap_frame_is_an_ensemble_of_the_fic_alone(pkg, mode):
    frame = pkg.fic_bootstrap_frame(mode)
    lay = pkg.Modulator.frontend_describe(frame)
    assert (lay["mode"], lay["nst"], lay["fic_bytes"], lay["fic_offset"]) == (mode, 0, 128 if mode == 3 else 96, 12)
    assert lay == pkg.Modulator.frontend_describe(synth_eti(1, subchannels=(), mid=FM.MID[mode])[0])
    pkg.decode_check_layout(frame)
    assert bytes(frame) == FM.make_header(dict(sub=[]), mode)
    with pytest.raises(pkg.DabGpuError, match="transmission mode not valid"):
        pkg.fic_bootstrap_frame(5)


def test_refusals_each_with_its_message(pkg):
    good = model_result(FC.with_fic(synth_eti(2, **ETI_CASES["multi"]["kw"]), 1), 1)
    pkg.fic_make_header(good, 1)

    def refused(res, match):
        assert FM.header_refusal(res) is None or match.startswith(FM.header_refusal(res)[:20])
        with pytest.raises(pkg.DabGpuError, match=match):
            pkg.fic_make_header(res, 1)

    none = copy.deepcopy(good)
    none.update(n_subch=0, sub=[])
    refused(none, "fic: no sub-channel organisation seen")
    many = copy.deepcopy(good)
    many["n_subch"] = 65
    refused(many, "fic: more than 64 sub-channels")
    changed = copy.deepcopy(good)
    changed["sub"][2]["changes"] = 1
    refused(changed, r"fic: sub-channel 2 was redefined inside the capture \(1 changes\)")
    refused(one_subch(FC.sub_short(7, 0, 3, switch=1)), "fic: sub-channel 7 is not supported: short form with the table switch set")
    refused(one_subch(FC.sub_long(8, 0, 2, 1, 48)), "fic: sub-channel 8 is not supported: long form with protection option 2")
    refused(one_subch(FC.sub_long(9, 0, 0, 2, 47)), "fic: sub-channel 9 is not supported: EEP size 47 is not a multiple of 6")
    over = FM.scan([FC.fib([FC.fig0_1([FC.sub_long(0, 0, 0, 2, 96), FC.sub_long(1, 95, 0, 2, 96)])])])[1]
    refused(over, "overlap at capacity unit 95")
    beyond = one_subch(FC.sub_long(3, 800, 0, 2, 96))
    refused(beyond, "FrameMultiplexer: sub-channel beyond the end of the CIF")
    with pytest.raises(pkg.DabGpuError, match="transmission mode not valid"):
        pkg.fic_make_header(good, 0)


def test_the_models_results_for_the_refused_shapes_say_why():
    """the model's own view of the two forms make_header refuses, and of a redefinition"""
    assert FM.scan([FC.fib([FC.fig0_1([FC.sub_short(7, 0, 3, switch=1)])])])[1]["sub"][0]["supported"] == 0
    assert FM.scan([FC.fib([FC.fig0_1([FC.sub_long(8, 0, 2, 1, 48)])])])[1]["sub"][0]["supported"] == 0
    a, b = FC.fib([FC.fig0_1([FC.sub_long(8, 0, 0, 2, 48)])]), FC.fib([FC.fig0_1([FC.sub_long(8, 0, 0, 2, 96)])])
    s = FM.scan([a, a, b, b, FC.fib()])[1]["sub"][0]
    assert (s["seen"], s["changes"], s["first_fib"], s["last_fib"], s["size_cu"]) == (4, 1, 0, 3, 96)


@pytest.mark.parametrize("name,fibs", [("cfg1", 144), ("multi", 129), ("mode2", 60), ("mode3", 80), ("mode4", 60)])
def test_the_pseudo_random_fic_of_the_existing_streams_has_no_good_fib(name, fibs):
    c = ETI_CASES[name]
    res = model_result(synth_eti(c["nframes"], **c["kw"]), c["mode"])
    assert (res["fibs"], res["fibs_ok"], res["fibs_bad"], res["fibs_zero"], res["n_subch"]) == (fibs, 0, fibs, 0, 0)


def test_a_fib_of_zeros_counts_as_zero_not_as_bad():
    recs, res = FM.scan([bytes(32), FC.fib(), FC.fib(crc=False), bytes(31) + b"\x01"])
    assert [r["flags"] for r in recs] == [FM.ZERO, FM.CRC_OK, 0, 0]
    assert (res["fibs"], res["fibs_ok"], res["fibs_bad"], res["fibs_zero"]) == (4, 1, 2, 1)
    assert FM.pack_record(recs[0]) == b"\x02" + bytes(287)
