"""The FIC reader on the device (include/dabgpu.h, "the FIC reader"; odr-dabmod_amd/csrc/fic.hip): FIB CRCs, the FIG walk, the
reduction to the sub-channel table -- BYTE equality of the result and of every record with the plain-Python model
(tests/fic_model.py) -- and the blind loop: a decoder that has only ever seen the NST = 0 bootstrap frame reads the FIC of a
signal, configures itself and returns the payload.  All integers, nothing to tolerate."""
import os
import subprocess

import numpy as np
import pytest

from tests import decode_cases as K
from tests import decode_model as M
from tests import fic_cases as FC
from tests import fic_model as FM
from tests.conftest import ROOT
from tests.golden.frontend_cases import ETI_CASES
from tests.golden.synth import synth_eti

pytestmark = pytest.mark.gpu

HOST = os.path.join(ROOT, "odr-dabmod_amd", "host")
G, F = 1, 2


@pytest.fixture(scope="module")
def mods(pkg):
    ms = {m: pkg.Modulator(mode=m, max_frames=20) for m in (1, 2, 3, 4)}
    yield ms
    for m in ms.values():
        m.close()


def entry(s, variant=0):
    """the FIG 0/1 entry of SubChId s: even ids in the short form, odd ones in the long form"""
    if s % 2 == 0:
        return FC.sub_short(s, 13 * s, (s + variant) % 64, switch=int(s % 16 == 14))
    return FC.sub_long(s, 13 * s, (s // 2) % 3, s % 4, 6 * (s + 1) + variant)


def mixed_fibs(n, seed=3):
    """n FIBs that cycle through every kind of content the walk distinguishes; all 64 SubChIds, in both forms, spread over them"""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        kind = i % 12
        some = [entry((5 * i + k) % 64) for k in range(3)]
        if kind == 0:                                   # clean: FIG 0/0 and FIG 0/1
            f = FC.fib([FC.fig0_0(0x4001 + (i > n // 2), change=i % 4, alarm=i % 2, cif_hi=i % 20, cif_lo=i % 250), FC.fig0_1(some)])
        elif kind == 1:                                 # services and a label
            comp = FC.component(3, 0, 0xABC, primary=0, ca=1) if i % 24 == 1 else FC.component(0, 63, i % 64)
            f = FC.fib([FC.fig0_2([FC.service(0x1000 + i % 7, [comp], local=1, caid=5)]),
                        FC.fig1(i % 2, 0x4001 if i % 2 == 0 else 0x1000 + i % 7, b"Label %d" % i)])
        elif kind == 2:                                 # one bit flipped: its entries must vanish
            f = FC.flip(FC.fib([FC.fig0_1(some)]), int(rs.randint(0, 256)))
        elif kind == 3:                                 # FIGs with C/N, OE or P/D set, beside one that counts
            f = FC.fib([FC.fig0_1(some[:1], cn=1), FC.fig0_0(0x7777, oe=1), FC.fig0_2([FC.service(1, [])], pd=1), FC.fig0_1(some[1:])])
        elif kind == 4:                                 # unknown types and extensions, empty FIGs
            f = FC.fib([FC.fig(2, b"\x01\x02\x03"), FC.fig0(5, b"\x11\x22"), FC.fig0(13, b"\x00" * 4), FC.fig(5, b"\x55"), FC.fig(0),
                        FC.fig(1), FC.fig(7, b"\x99" * 2), FC.fig0_1(some[:1])])
        elif kind == 5:                                 # a FIG whose length runs past byte 29, behind one that counts
            body = FC.fig0_1(some[:2]) + bytes([0 << 5 | 31, 1]) + bytes(rs.randint(0, 256, 24).astype(np.uint8))
            body = body[:30]
            c = FM.crc16(body)
            f = body + bytes([c >> 8, c & 0xFF])
        elif kind == 6:                                 # a FIG 0/1 whose last entry is cut
            f = FC.fib([FC.fig0_1([entry(1), entry(3)[:3]]), FC.fig0_1([entry(2), entry(4)[:2]]), FC.fig0_1([entry(6)])])
        elif kind == 7:                                 # exactly full, no end marker: 2 + 28 bytes
            f = FC.fib([FC.fig0_1([entry((7 * i + k) % 64 | 1) for k in range(7)])])
            assert len(FC.fig0_1([entry(1)] * 7)) == 30
        elif kind == 8:                                 # zero
            f = bytes(32)
        elif kind == 9:                                 # nine short entries: a full record
            f = FC.fib([FC.fig0_1([entry((2 * (i + k)) % 64) for k in range(9)])])
        elif kind == 10:                                # more services and labels than a record keeps
            f = FC.fib([FC.fig0_2([FC.service(0x2000 + k, [FC.component(1, 5, k)]) for k in range(5)])]) if i % 24 == 10 else \
                FC.fib([FC.fig0_2([FC.service(0x3000, [FC.component(0, 0, k) for k in range(5)]),
                                   FC.service(0x3001, [FC.component(2, 1, k) for k in range(4)])])])
        else:                                           # only the end marker; a label of a component; one of another ensemble
            f = (FC.fib(), FC.fib([FC.fig1(4, 0x1234, b"component")]), FC.fib([FC.fig1(1, 0x1000, b"elsewhere", oe=1)]))[(i // 12) % 3]
        out.append(f)
    return out


def compare(md, fibs, images, fic_offset, device=False):
    """the scan of `images` against the model run on `fibs`: the result's bytes and every record's"""
    if device:
        import torch
        d = torch.from_numpy(images).cuda()
        md.fic_scan_dev(d, images.shape[0], fic_offset)
    else:
        md.fic_scan(images, fic_offset)
    recs, res = FM.scan(fibs)
    got = md.fic_records()
    assert got.shape == (len(fibs), FM.RECORD_BYTES)
    for i, r in enumerate(recs):
        assert bytes(got[i]) == FM.pack_record(r), ("record", i, fibs[i].hex())
    assert md.fic_result_bytes() == FM.pack_result(res)
    assert res["fibs_ok"] + res["fibs_bad"] + res["fibs_zero"] == res["fibs"] == len(fibs)
    return recs, res


# --------------------------------------------------------------------------- 1. the kernels against the model
@pytest.mark.parametrize("mode,n_images", [(1, 1), (1, 22), (1, 86), (3, 1), (3, 65)])
def test_scan_of_raw_images_equals_the_model(mods, mode, n_images):
    """3, 66 and 258 FIBs in Mode I (a wave, a 256-lane workgroup and beyond), 4 and 260 in Mode III; the FIC at an offset that
    is only four-byte aligned"""
    per = 4 if mode == 3 else 3
    fibs = mixed_fibs(n_images * per, seed=mode)
    images = FC.images_of(fibs, fic_offset=28, fibs_per_image=per)
    recs, res = compare(mods[mode], fibs, images, 28, device=n_images > 1)
    if n_images == 1:
        return
    flipped = [i for i in range(len(fibs)) if i % 12 == 2]
    assert res["fibs_bad"] == len(flipped) and all(recs[i]["flags"] == 0 and not recs[i]["sub"] for i in flipped)
    assert res["fibs_zero"] == len(range(8, len(fibs), 12)) and res["figs_truncated"] == len(range(5, len(fibs), 12))
    assert res["fig0_skipped"] == 3 * len(range(3, len(fibs), 12)) and res["figs_type"][7] and res["fig0_ext"][13]
    assert res["services_dropped"] and res["components_dropped"]
    if len(fibs) > 200:
        assert [s["subchid"] for s in res["sub"]] == list(range(64)) and {s["form"] for s in res["sub"]} == {0, 1}
    head = mods[mode].fic_result()
    assert head["n_subch"] == res["n_subch"] and head["sub"] == [{k: s[k] for k in FM.SUBCH_FIELDS} for s in res["sub"]]
    ens, svcs = mods[mode].fic_services()
    want_ens, want_svcs = FM.services(recs)
    assert svcs == want_svcs and ens == want_ens and len(svcs) > 3


@pytest.mark.parametrize("at", [129, 64, 256, 63, 257])
def test_a_redefinition_gives_one_change_wherever_it_falls(pkg, mods, at):
    """258 FIBs that all define SubChId 5 (and the EId): redefined halfway, on a wave boundary, on a workgroup boundary and one
    FIB beside them -- one change, the first and the last FIB, the last definition"""
    a, b = FC.sub_long(5, 100, 0, 2, 96), FC.sub_long(5, 100, 0, 2, 48)
    fibs = [FC.fib([FC.fig0_0(0x4001 if i < at else 0x4002), FC.fig0_1([entry(9), a if i < at else b])]) for i in range(258)]
    recs, res = compare(mods[1], fibs, FC.images_of(fibs), 12, device=True)
    s = [x for x in res["sub"] if x["subchid"] == 5][0]
    assert (s["seen"], s["changes"], s["first_fib"], s["last_fib"], s["size_cu"], s["bitrate"]) == (258, 1, 0, 257, 48, 64)
    assert (res["eid"], res["eid_seen"], res["eid_changes"], res["eid_first_fib"], res["eid_last_fib"]) == (0x4002, 258, 1, 0, 257)
    assert [x["changes"] for x in res["sub"] if x["subchid"] == 9] == [0]
    with pytest.raises(pkg.DabGpuError, match="sub-channel 5 was redefined inside the capture"):
        mods[1].configure_from_fic()


# --------------------------------------------------------------------------- 2. repeatability
def test_the_same_input_gives_the_same_bytes_from_host_and_device_pointers(mods):
    import torch
    md = mods[1]
    fibs = mixed_fibs(258, seed=9)
    images = FC.images_of(fibs, fic_offset=40)
    runs = []
    d = torch.from_numpy(images).cuda()
    for how in ("host", "device", "device", "host"):
        if how == "host":
            md.fic_scan(images, 40)
        else:
            md.fic_scan_dev(d, images.shape[0], 40)
        runs.append((md.fic_result_bytes(), md.fic_records().tobytes()))
    assert all(r == runs[0] for r in runs[1:])
    assert runs[0][0] == FM.pack_result(FM.scan(fibs)[1])


def test_refusals(pkg, mods):
    md = pkg.Modulator(mode=1, max_frames=1)
    try:
        images = FC.images_of(mixed_fibs(3))
        with pytest.raises(pkg.DabGpuError, match="no FIC scan"):
            md.fic_result()
        with pytest.raises(pkg.DabGpuError, match="no FIC scan"):
            md.configure_from_fic()
        with pytest.raises(pkg.DabGpuError, match="needs a configured front-end"):
            md.fic_scan(images)
        with pytest.raises(pkg.DabGpuError, match="multiple of 4"):
            md.fic_scan(images, 14)
        with pytest.raises(pkg.DabGpuError, match="exceeds the 6144-byte image"):
            md.fic_scan(images, 6144 - 92)
        with pytest.raises(pkg.DabGpuError, match="n_images must lie in"):
            md.fic_scan(images[:0], 12)
        with pytest.raises(pkg.DabGpuError, match="no FIC scan"):
            md.fic_records()
        assert md.fic_scan(images, 6144 - 96)["fibs"] == 3
        md.frontend_configure(pkg.fic_bootstrap_frame(1))
        assert md.fic_scan(images)["fibs_ok"] == FM.scan(mixed_fibs(3))[1]["fibs_ok"]
        with pytest.raises(pkg.DabGpuError, match="no sub-channel organisation seen"):
            md.fic_scan(FC.images_of([FC.fib()] * 3))
            md.configure_from_fic()
    finally:
        md.close()


# --------------------------------------------------------------------------- 3. the blind loop
def blind_stream(name, subchids=None):
    """20 ETI frames of the case's layout from FP = 0 with a FIC that says so"""
    if name == "stc_order":
        mode, subs = 1, K.SHAPES["stc_order_is_not_sad_order"]
    else:
        mode, subs = ETI_CASES[name]["mode"], ETI_CASES[name]["kw"].get("subchannels", ((0, 48, 0x22),))
    return mode, FC.with_fic(synth_eti(20, subchannels=subs, mid=K.MID[mode], seed=77), mode, subchids)


def received_bits(pkg, mode, eti):
    """ETI -> IQ (GainControl, FIRFilter) on one context -> demodulated: the coded bits a receiver has"""
    tx = pkg.Modulator(mode=mode, max_frames=20)
    try:
        tx.set_gain(2, 1.0, 1.0 / 50000.0, 4.0)
        tx.set_fir_taps(None)
        tx.frontend_configure(eti[0])
        return tx.demod(tx.chain_eti(eti, G | F), early=44)
    finally:
        tx.close()


@pytest.mark.parametrize("name", ["cfg1", "multi", "mode2", "mode3", "mode4", "stc_order"])
def test_blind_loop_configures_itself_and_returns_the_payload(pkg, name):
    """ETI -> IQ -> coded bits on one context; a SECOND context that only ever saw fic_bootstrap_frame: decode -> fic_scan_dev
    (past the fifteen lead-in images) -> configure_from_fic -> decode again.  stc_order: the FIC numbers the sub-channels 5, 1, 3
    in STC order, so the header made from it lists them in another order than the original frame -- the payload is compared
    per sub-channel through each layout's own offsets."""
    import torch
    subchids = (5, 1, 3) if name == "stc_order" else None
    mode, eti = blind_stream(name, subchids)
    bits = received_bits(pkg, mode, eti)
    n_tf, n = bits.shape[0], 20
    assert n_tf * M.CIFS[mode] == n
    original = pkg.Modulator.frontend_describe(eti[0])
    rx = pkg.Modulator(mode=mode, max_frames=n_tf)
    try:
        rx.frontend_configure(pkg.fic_bootstrap_frame(mode))
        d_bits = torch.from_numpy(np.ascontiguousarray(bits)).cuda()
        d_out = torch.zeros(n * 6144, dtype=torch.uint8, device="cuda")
        rx.decode_dev(d_bits, n_tf, d_out)
        rx.fic_scan_dev(d_out[15 * 6144:], n - 15)
        res = rx.fic_result()
        fic_bytes = 128 if mode == 3 else 96
        want = FM.scan(FM.fibs_of(eti[:n - 15], original["fic_offset"], fic_bytes))[1]
        assert res["fibs_bad"] == 0 and res["fibs_zero"] == 0 and res["fibs_ok"] == want["fibs_ok"] == (n - 15) * fic_bytes // 32
        assert rx.fic_result_bytes() == FM.pack_result(want) and res["eid"] == 0x4FFF
        found = pkg.Modulator.frontend_describe(pkg.fic_make_header(res, mode))
        rx.configure_from_fic()
        # the sub-channel of the original layout that each one of the found layout is: the same start address
        match = [[s["sad"] for s in original["subchannels"]].index(t["sad"]) for t in found["subchannels"]]
        if subchids is None:
            assert found == original and match == list(range(original["nst"]))
        else:
            assert match == [1, 2, 0] and found["fic_offset"] == original["fic_offset"]
        ref = np.zeros((n, 6144), np.uint8)
        fo = found["fic_offset"]
        ref[15:, fo:fo + fic_bytes] = eti[:n - 15, fo:fo + fic_bytes]
        for t, i in zip(found["subchannels"], match):
            o = original["subchannels"][i]
            assert {k: t[k] for k in t if k != "offset"} == {k: o[k] for k in o if k != "offset"}
            ref[15:, t["offset"]:t["offset"] + t["framesize"]] = eti[:n - 15, o["offset"]:o["offset"] + o["framesize"]]
        d_ref = torch.from_numpy(ref).cuda()
        d_out.zero_()
        rx.decode_dev(d_bits, n_tf, d_out, d_ref)
        images = d_out.cpu().numpy().reshape(n, 6144)
        keep = M.payload_mask(found)
        assert np.array_equal(images[15:][:, keep], ref[15:][:, keep]) and not images[:15].any()
        for i in range(n):
            for unit in range(1 + found["nst"]):
                st = rx.decode_stats(i, unit)
                assert st["valid"] == int(i >= 15) and st["bit_errors"] == 0 and (st["n_bits"] > 0) == (i >= 15), (i, unit)
        ens, svcs = rx.fic_services()
        first = min(original["nst"], 4)                     # (with_fic: one FIG 0/2 with four services, as many as a record keeps)
        assert [s["sid"] for s in svcs][:first] == [0x1000 + k for k in (subchids or range(original["nst"]))][:first]
        assert ens["text"] == b"Ensemble".ljust(16) and ens["id"] == 0x4FFF
    finally:
        rx.close()


# --------------------------------------------------------------------------- 4. damaged bits
@pytest.mark.parametrize("rate,seed", [(0.04, 1), (0.12, 1)])
def test_damaged_bits_never_configure_a_wrong_layout(pkg, mods, rate, seed):
    """dense_flips on the coded bits.  The scan of the decoder's output must equal the model run on THOSE SAME output bytes: this
    is not an independent check of the decoder, only of the reader behind it.  configure_from_fic either succeeds with the true
    layout or refuses.  At the existing 4 % (seed 1) the FIC's rate-1/3 code corrects everything: 15 good FIBs of 15, as the
    numpy decoder gives for seeds 1 ... 7.  So that good AND bad FIBs occur, a second case at 12 % (seed 1; chosen on the CPU
    with tests/decode_model.py: 10 good, 5 bad)."""
    eti = FC.with_fic(synth_eti(20, subchannels=K.MULTI, mid=1), 1)
    bits = K.cpu_front_end().eti_to_bits(eti, 1)
    noisy = bits ^ K.dense_flips(bits.shape, seed=seed, rate=rate)
    md = mods[1]
    md.frontend_configure(pkg.fic_bootstrap_frame(1))
    images, _ = md.decode(noisy)
    res = md.fic_scan(images)
    want = FM.scan(FM.fibs_of(images, 12, 96))[1]
    assert md.fic_result_bytes() == FM.pack_result(want)
    assert res["fibs_ok"] + res["fibs_bad"] + res["fibs_zero"] == res["fibs"] == 60 and res["fibs_zero"] == 45
    print("damaged bits, rate %.2f seed %d: %d good, %d bad FIBs" % (rate, seed, res["fibs_ok"], res["fibs_bad"]))
    assert (res["fibs_ok"], res["fibs_bad"]) == ((15, 0) if rate == 0.04 else (10, 5))
    true_layout = pkg.Modulator.frontend_describe(eti[0])
    try:
        made = pkg.fic_make_header(res, 1)
        md.configure_from_fic()
    except pkg.DabGpuError:
        return
    assert pkg.Modulator.frontend_describe(made) == true_layout


# --------------------------------------------------------------------------- 5. dabmod_file --loopback --blind
def _dabmod_file(fin, fout, opts):
    return subprocess.run([os.path.join(HOST, "dabmod_file"), fin, fout] + opts, capture_output=True, text=True, timeout=300)


def test_dabmod_file_blind_reads_its_configuration_from_the_fic(tmp_path):
    """40 frames in Mode I, batches of five transmission frames: the first batch leaves five images to read the FIC from"""
    fin, fout = str(tmp_path / "in.eti"), str(tmp_path / "out")
    FC.with_fic(synth_eti(40, subchannels=K.MULTI, mid=1), 1).tofile(fin)
    r = _dabmod_file(fin, fout, ["--gpu-frontend", "--loopback", "--blind", "--batch", "5", "--fir", "default"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "blind: 60 FIBs: 15 good, 0 bad, 45 zero; EId 0x4FFF; 5 sub-channels" in r.stderr
    assert "blind: SubChId  1: start 100 CU, size  42 CU, EEP 2-B,  64 kbit/s (TPL 0x25, STL 24)" in r.stderr
    assert "blind: SubChId  4: start 400 CU, size 416 CU, UEP 1, 384 kbit/s (TPL 0x00, STL 144)" in r.stderr
    layout_bits = 8 * (96 + 8 * sum(s[1] for s in K.MULTI))
    assert "loopback: 25 frames compared, 0 FIC and 0 MSC payload bit errors in %d bits, 0 corrected" % (25 * layout_bits) in r.stderr


def test_dabmod_file_blind_exits_4_on_a_pseudo_random_fic(tmp_path):
    fin, fout = str(tmp_path / "in.eti"), str(tmp_path / "out")
    synth_eti(40, subchannels=K.MULTI, mid=1).tofile(fin)
    r = _dabmod_file(fin, fout, ["--gpu-frontend", "--loopback", "--blind", "--batch", "5", "--fir", "default"])
    assert r.returncode == 4, r.stderr[-2000:]
    assert "blind: 60 FIBs: 0 good, 15 bad, 45 zero" in r.stderr and "no configuration could be read" in r.stderr
    r = _dabmod_file(fin, fout, ["--gpu-frontend", "--blind"])
    assert r.returncode == 2 and "--blind does not go without --loopback" in r.stderr
