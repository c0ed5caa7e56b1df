"""The superframe reader on the device (include/dabgpu.h, "the superframe reader"; odr-dabmod_amd/csrc/superframe.hip): BYTE equality
of every candidate's record, of the corrected bytes and of the call's result with the plain-Python model (tests/superframe_model.py,
itself held to the reference's Reed-Solomon code by tests/test_superframe_cpu.py) run on the same input bytes; the call behind a
decoder on the lanes; the loop through modulator, channel, soft demodulator and soft decoder; dabmod_file --superframe.
All integers, nothing to tolerate."""
import os
import subprocess

import numpy as np
import pytest

from tests import decode_cases as K
from tests import superframe_cases as SC
from tests import superframe_model as SM
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

HOST = os.path.join(ROOT, "odr-dabmod_amd", "host")


@pytest.fixture(scope="module")
def md(pkg):
    m = pkg.Modulator(mode=2, max_frames=45)
    yield m
    m.close()


def compare(pkg, md, images, offset, s, device=True):
    """one call on `images` against the model on the same bytes: every record, the output bytes, the result -> (records, out, result)"""
    images = np.ascontiguousarray(images, np.uint8).reshape(-1, 6144)
    n = images.shape[0]
    if device:
        import torch
        d_out = torch.zeros((n - 4) * 110 * s, dtype=torch.uint8, device="cuda")
        assert md.superframe_dev(torch.from_numpy(images).cuda(), n, offset, 24 * s, d_out) == d_out.numel()
        out, res = d_out.cpu().numpy(), md.superframe_result()
    else:
        out, res = md.superframe(images, offset, 24 * s)
    got = md.superframe_records()
    recs, want_out = SM.scan(images, offset, 24 * s)
    assert got.shape == (n - 4, SM.RECORD_BYTES)
    for f, r in enumerate(recs):
        assert bytes(got[f]) == SM.pack_record(r), ("record", f, SM.unpack_record(got[f]), r)
        assert pkg.superframe_record_dict(got[f]) == r
    assert out.tobytes() == want_out
    assert res == SM.walk(recs)
    return recs, want_out, res


# --------------------------------------------------------------------------- 7. shapes
OFFSETS = {1: 0, 3: 6144 - 72, 4: 12 + 4 * 1 + 96, 9: 2052, 24: 6144 - 576}


@pytest.mark.parametrize("n_images", [5, 9, 23])
@pytest.mark.parametrize("s", [1, 3, 4, 9, 24])
def test_clean_superframes_at_every_size_and_phase(pkg, md, s, n_images):
    """One word at stride 1 up to 24 words (the four waves loop six times); 1, 5 and 19 candidates; the superframes from image 0, 2
    or 4 on; random bytes everywhere else, the sub-channel's frames in front of and behind the superframes included (their
    candidates are uncorrectable words: the model says which).  The sub-channel first in the image, last in it (s = 3, 24) and
    behind one STC word and the FIC (s = 4).  The host-pointer entry at n = 9."""
    phase = 0 if n_images == 5 else (0, 2, 4)[(s + n_images) % 3]
    images, placed = SM.stream_images(n_images, s, OFFSETS[s], phase, seed=100 * s + n_images,
                                      **dict(zip(("dac_rate", "sbr_flag"), ((1, 0), (0, 1), (1, 1), (0, 0))[s % 4])))
    recs, out, res = compare(pkg, md, images, OFFSETS[s], s, device=n_images != 9)
    assert [f for f, _ in placed] == list(range(phase, n_images - 4, 5)) and placed
    for f, _ in placed:
        assert SM.accepted(recs[f]) and recs[f]["rs_corrected"] == 0 and recs[f]["rs_failed"] == 0 and recs[f]["cw_errors"] == [0] * 24
        assert recs[f]["au_ok"] == (1 << recs[f]["num_aus"]) - 1
    assert set(f for f, _ in placed) <= set(res["accepted"]) and res["rs_corrected"] == 0
    if res["accepted"] == [f for f, _ in placed]:                  # (a random candidate passes the Fire code once in 2^16)
        aus, ok = pkg.superframe_aus(out, res, md.superframe_records())
        assert aus == [a for _, sf in placed for a in sf] and all(ok)


# --------------------------------------------------------------------------- 8. errors
def error_mask(n_images, s, offset, placed, seed):
    """an xor mask over the images: word i of superframe k gets (i + k) mod 6 byte errors in the first superframes and 6 ... 8 in
    every third word of the last one; the first errors of a word on the edge positions.  -> (mask, {(first image, word): count})"""
    rs = np.random.RandomState(seed)
    mask = np.zeros((n_images, 6144), np.uint8)
    counts = {}
    for k, (f, _) in enumerate(placed):
        sub = np.zeros(SM.N * s, np.uint8)
        for i in range(s):
            n_err = (i + k) % 6
            if k == len(placed) - 1 and i % 3 == 0:
                n_err = 6 + (i // 3) % 3
            pos = list(SC.EDGES[(i + k) % 6:] + SC.EDGES[:(i + k) % 6])[:n_err]
            while len(pos) < n_err:
                p = int(rs.randint(0, SM.N))
                if p not in pos:
                    pos.append(p)
            for p in pos:
                sub[i + s * p] = rs.randint(1, 256)
            counts[(f, i)] = n_err
        mask[f:f + 5, offset:offset + 24 * s] = sub.reshape(5, 24 * s)
    return mask, counts


@pytest.mark.parametrize("s,n_images", [(5, 20), (24, 15)])
def test_seeded_errors_injected_on_the_device(pkg, md, s, n_images):
    """0 ... 5 errors per word, positions 0, 63, 64, 109, 110, 119 among them (both lane halves, the data / parity seam, both ends),
    the header's words included so that the Fire code passes only after correction; 6 ... 8 in some words of the last superframe."""
    import torch
    offset = 400
    images, placed = SM.stream_images(n_images, s, offset, 0, seed=7 * s)
    mask, counts = error_mask(n_images, s, offset, placed, seed=s)
    d = torch.from_numpy(images).cuda() ^ torch.from_numpy(mask).cuda()
    noisy = d.cpu().numpy()
    assert np.array_equal(noisy, images ^ mask)
    recs, out, res = compare(pkg, md, noisy, offset, s)
    last = placed[-1][0]
    for f, aus in placed[:-1]:
        want = [counts[(f, i)] for i in range(s)]
        assert recs[f]["cw_errors"][:s] == want and recs[f]["rs_corrected"] == sum(want) and recs[f]["rs_max"] == max(want)
        assert SM.accepted(recs[f]) and recs[f]["au_ok"] == (1 << recs[f]["num_aus"]) - 1
        raw = bytes(noisy[f, offset:offset + 11])                   # as received, the header fails its Fire code
        assert SM.fire_crc(raw[2:]) != (raw[0] << 8 | raw[1])
    assert recs[last]["rs_failed"] >= 1 and recs[last]["flags"] & SM.RS_FAILED
    assert [recs[last]["cw_errors"][i] for i in range(s) if i % 3] == [counts[(last, i)] for i in range(s) if i % 3]
    assert res["accepted"][:len(placed) - 1] == [f for f, _ in placed[:-1]]


def test_the_fixtures_words_through_the_kernel(pkg, md):
    """tests/golden/superframe_rs.json laid out as sub-channels of s = 8, one group of eight corrupted words per five images: what
    lib/fec made of each word -- its count and bytes for the corrected and the miscorrected ones -- and 0xFF with the bytes kept
    for the refused ones AND for those with a root in the padding"""
    s, offset = 8, 1000
    groups = SC.golden_subchannel(SC.golden(), s)
    assert len(groups) >= 20
    rs = np.random.RandomState(8)
    images = rs.randint(0, 256, (5 * len(groups), 6144)).astype(np.uint8)
    for g, (buf, _) in enumerate(groups):
        images[5 * g:5 * g + 5, offset:offset + 24 * s] = np.frombuffer(buf, np.uint8).reshape(5, 24 * s)
    recs, out, _ = compare(pkg, md, images, offset, s)
    kinds = set()
    for g, (buf, part) in enumerate(groups):
        r, o = recs[5 * g], out[5 * g * 110 * s:(5 * g + 1) * 110 * s]
        for i, e in enumerate(part):
            kind = SC.classify(e["ret"], e["loc"])
            kinds.add(kind)
            if kind == "corrected":
                assert r["cw_errors"][i] == e["ret"] and o[i::s] == bytes.fromhex(e["after"])[:110], (g, i)
            else:
                assert r["cw_errors"][i] == SM.FAILED and o[i::s] == bytes.fromhex(e["bad"])[:110], (g, i, kind)
    assert kinds == {"corrected", "refused", "padding"}


# --------------------------------------------------------------------------- 9. geometry independence
def test_one_call_and_overlapping_calls_give_the_same_records_bytes_and_walk(pkg, md):
    """300 images (s = 4, superframes from image 3 on, sparse byte errors) in one call, and as calls of 64 + 4 images that overlap
    by four: candidate f's record and bytes are the same, and the walk over the merged records is the one call's result"""
    import torch
    s, offset, n = 4, 112, 300
    images, placed = SM.stream_images(n, s, offset, 3, seed=300)
    rs = np.random.RandomState(301)
    hit = rs.random_sample(images.shape) < 0.01
    hit[:, :offset] = hit[:, offset + 24 * s:] = False
    images[hit] ^= rs.randint(1, 256, int(hit.sum())).astype(np.uint8)
    d = torch.from_numpy(images).cuda()
    d_out = torch.zeros((n - 4) * 110 * s, dtype=torch.uint8, device="cuda")
    md.superframe_dev(d, n, offset, 24 * s, d_out)
    whole_rec, whole_out, whole_res = md.superframe_records(), d_out.cpu().numpy(), md.superframe_result()
    recs, outs = [], []
    for a in range(0, n - 4, 64):
        k = min(68, n - a)
        d_part = torch.zeros((k - 4) * 110 * s, dtype=torch.uint8, device="cuda")
        md.superframe_dev(d[a:a + k], k, offset, 24 * s, d_part)
        recs.append(md.superframe_records())
        outs.append(d_part.cpu().numpy())
    assert np.array_equal(np.concatenate(recs), whole_rec) and np.array_equal(np.concatenate(outs), whole_out)
    merged = SM.walk([SM.unpack_record(r) for r in np.concatenate(recs)])
    assert merged == whole_res and whole_res["superframes"] >= 50 and whole_res["first"] == 3 and whole_res["rs_corrected"] > 100
    sample = list(range(0, 40)) + list(range(250, 296))                         # the model on both ends (the rest: equal to each other)
    for f in sample:
        r, o = SM.candidate(images[f:f + 5, offset:offset + 24 * s].tobytes(), s)
        assert bytes(whole_rec[f]) == SM.pack_record(r) and whole_out[f * 110 * s:(f + 1) * 110 * s].tobytes() == o, f


# --------------------------------------------------------------------------- 10. lanes
def test_queued_behind_the_decoder_whose_output_it_reads(pkg):
    """decode_dev then superframe_dev on its output with no host wait in between -- queued on the context's own stream, and on a
    caller's stream -- against the same two calls with a wait in between"""
    import torch
    eti, placed = SC.loop_stream()
    bits = K.cpu_front_end().eti_to_bits(eti, SC.LOOP_MODE)
    n = SC.LOOP_FRAMES
    m = pkg.Modulator(mode=SC.LOOP_MODE, max_frames=n)
    try:
        m.frontend_configure(eti[0])
        d_bits = torch.from_numpy(np.ascontiguousarray(bits)).cuda()
        side = torch.cuda.Stream()
        runs = {}
        for how in ("waited", "queued", "stream", "waited"):
            d_img = torch.zeros(n * 6144, dtype=torch.uint8, device="cuda")
            d_out = torch.zeros(26 * 110 * SC.LOOP_S, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            m.decode_reset()
            if how == "waited":
                m.decode_dev(d_bits, n, d_img)
                m.synchronize()
                m.superframe_dev(d_img[15 * 6144:], n - 15, SC.LOOP_OFFSET, SC.LOOP_FRAMESIZE, d_out)
            elif how == "queued":
                m.decode_dev(d_bits, n, d_img, queued=True)
                m.superframe_dev(d_img[15 * 6144:], n - 15, SC.LOOP_OFFSET, SC.LOOP_FRAMESIZE, d_out, queued=True)
            else:
                with torch.cuda.stream(side):
                    m.decode_dev(d_bits, n, d_img, stream=side.cuda_stream)
                    m.superframe_dev(d_img[15 * 6144:], n - 15, SC.LOOP_OFFSET, SC.LOOP_FRAMESIZE, d_out, stream=side.cuda_stream)
            got = (m.superframe_result(), m.superframe_records().tobytes())
            torch.cuda.synchronize()
            got += (d_out.cpu().numpy().tobytes(),)
            assert runs.setdefault("first", got) == got, how
        res = runs["first"][0]
        assert res["accepted"] == SC.LOOP_ACCEPTED and res["aus_bad"] == 0 and res["aus"] == 6 * 5 and res["rs_corrected"] == 0
    finally:
        m.close()


def test_refusals(pkg, md):
    import torch
    fresh = pkg.Modulator(mode=2, max_frames=1)
    try:
        with pytest.raises(pkg.DabGpuError, match="no superframe call"):
            fresh.superframe_result()
        with pytest.raises(pkg.DabGpuError, match="no superframe call"):
            fresh.superframe_records()
    finally:
        fresh.close()
    images, _ = SM.stream_images(9, 2, 0, 0, seed=1)
    _, res = md.superframe(images, 0, 48)
    for args, why in [((images[:4], 0, 48), "n_images must lie in 5"), ((images, 0, 50), "framesize must be 24 s"),
                      ((images, 2, 48), "multiple of 4"), ((images, 6100, 48), "exceeds the 6144-byte image")]:
        with pytest.raises(pkg.DabGpuError, match=why):
            md.superframe(*args)
    d = torch.from_numpy(images).cuda()
    with pytest.raises(pkg.DabGpuError, match="aligned to four bytes"):
        md.superframe_dev(d.reshape(-1)[1:], 8, 0, 48, torch.zeros(4 * 220, dtype=torch.uint8, device="cuda"))
    with pytest.raises(pkg.DabGpuError, match="output buffer too small"):
        md.superframe_dev(d, 9, 0, 48, torch.zeros(5 * 220 - 1, dtype=torch.uint8, device="cuda"))
    assert md.superframe_result() == res                                        # the previous result stays


def test_dabplus_subchannels_lead_from_the_fic_to_the_superframes_of_raw_eti_frames(pkg, md):
    """the loop's stream with a real FIC, as raw ETI frames: the FIC names sub-channel 0 as DAB+ audio (TMId 0, ASCTy 63), the
    configured layout says where it lies, and the reader finds every superframe of the file there"""
    from tests import fic_cases as FC
    eti, placed = SC.loop_stream()
    eti = FC.with_fic(eti, SC.LOOP_MODE)
    md.frontend_configure(eti[0])
    md.fic_scan(eti[:20])
    subs = md.dabplus_subchannels()
    assert subs == [dict(sid=0x1000, subchid=0, bitrate=32, index=0, offset=SC.LOOP_OFFSET, framesize=SC.LOOP_FRAMESIZE)]
    out, res = md.superframe(eti, subs[0]["offset"], subs[0]["framesize"])
    assert res["accepted"] == [f for f, _ in placed] == list(range(2, 40, 5)) and res["aus_bad"] == 0 and res["phase_changes"] == 0
    aus, ok = pkg.superframe_aus(out, res, md.superframe_records())
    assert aus == [a for _, sf in placed for a in sf] and all(ok)


# --------------------------------------------------------------------------- 11. the loop
@pytest.fixture(scope="module")
def loop(pkg):
    eti, placed = SC.loop_stream()
    lp = SC.Loop(pkg, eti)
    yield lp, placed
    lp.close()


def check_loop_against_model(pkg, got, placed):
    recs, out = SM.scan(got["images"], SC.LOOP_OFFSET, SC.LOOP_FRAMESIZE)
    assert [bytes(r) for r in got["records"]] == [SM.pack_record(r) for r in recs] and got["out"].tobytes() == out
    assert got["result"] == SM.walk(recs)
    aus, ok = pkg.superframe_aus(got["out"], got["result"], got["records"])
    sent = [a for f, sf in placed if f in SC.LOOP_ACCEPTED for a in sf]
    assert got["result"]["accepted"] == SC.LOOP_ACCEPTED and aus == sent and all(ok) and len(sent) == 30
    assert got["result"]["aus_ok"] == 30 and got["result"]["aus_bad"] == 0 and got["result"]["rs_failed"] == 0


def test_loop_clean_channel(pkg, loop):
    lp, placed = loop
    got = lp.run()
    check_loop_against_model(pkg, got, placed)
    assert got["bit_errors"] == 0 and got["result"]["rs_corrected"] == 0


@pytest.fixture(scope="module")
def noisy(loop):
    lp, _ = loop
    return lp.run(SC.LOOP_CN_DB, SC.LOOP_SEED)


def test_loop_noisy_channel_the_outer_code_copes(pkg, loop, noisy):
    """At the point of profiles/superframe.txt the soft decoder leaves payload bit errors, the outer code corrects them all with at
    most 3 corrections in a word (two of margin under t = 5), and every AU passes with the bytes that were sent.  The records are the
    model's on the decoder's own bytes: not an independent check of the decoder, only of the reader behind it."""
    _, placed = loop
    r = noisy["result"]
    print("C/N %.2f dB, seed %d: %d payload bit errors, %d RS bytes corrected, at most %d in a word, %d words failed, AUs %d ok / %d bad"
          % (SC.LOOP_CN_DB, SC.LOOP_SEED, noisy["bit_errors"], r["rs_corrected"], r["rs_max"], r["rs_failed"], r["aus_ok"], r["aus_bad"]))
    assert noisy["bit_errors"] > 0 and r["rs_corrected"] > 0 and r["rs_failed"] == 0 and r["rs_max"] <= 3
    check_loop_against_model(pkg, noisy, placed)


# --------------------------------------------------------------------------- 12. dabmod_file --superframe
def _dabmod_file(fin, fout, opts):
    return subprocess.run([os.path.join(HOST, "dabmod_file"), fin, fout] + opts, capture_output=True, text=True, timeout=300)


LOOP_OPTS = ["--gpu-frontend", "--mode", "%d" % SC.LOOP_MODE, "--batch", "%d" % SC.LOOP_FRAMES, "--fir", "default", "--loopback", "--soft"]


def test_dabmod_file_superframe_verdict_is_the_aus(tmp_path, noisy):
    """the noisy loop on the same file: with --superframe exit 0 and the Python run's figures, without it exit 2 as before"""
    fin = str(tmp_path / "in.eti")
    SC.loop_stream()[0].tofile(fin)
    noise = ["--channel-cn", "%.2f" % SC.LOOP_CN_DB, "--channel-seed", "%d" % SC.LOOP_SEED]
    r = _dabmod_file(fin, str(tmp_path / "out"), LOOP_OPTS + noise + ["--superframe", "0"])
    print(r.stderr[-900:])
    assert r.returncode == 0, r.stderr[-2000:]
    res = noisy["result"]
    assert ("superframe: sub-channel 0, 26 candidates, 5 superframes (first at 2), AUs 30 ok / 0 bad, %d RS bytes corrected (at most %d in a "
            "word), 0 words failed" % (res["rs_corrected"], res["rs_max"])) in r.stderr
    line = [ln for ln in r.stderr.splitlines() if "frames compared" in ln][0]
    assert int(line.split(" FIC and ")[1].split(" MSC")[0]) == noisy["bit_errors"] > 0
    r = _dabmod_file(fin, str(tmp_path / "out2"), LOOP_OPTS + noise)
    assert r.returncode == 2 and "superframe:" not in r.stderr, r.stderr[-2000:]


def test_dabmod_file_superframe_finds_nothing_in_random_bytes_and_carries_images_across_batches(tmp_path):
    fin = str(tmp_path / "in.eti")
    SC.loop_stream(random_payload=True)[0].tofile(fin)
    r = _dabmod_file(fin, str(tmp_path / "out"), LOOP_OPTS + ["--superframe", "0"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "superframe: sub-channel 0, 26 candidates, 0 superframes (first at -1), AUs 0 ok / 0 bad" in r.stderr
    # batches of 9 frames: the same candidates, four images carried from batch to batch
    SC.loop_stream()[0].tofile(fin)
    opts = [o if o != "%d" % SC.LOOP_FRAMES else "9" for o in LOOP_OPTS]
    r = _dabmod_file(fin, str(tmp_path / "out"), opts + ["--superframe", "0"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "superframe: sub-channel 0, 26 candidates, 5 superframes (first at 2), AUs 30 ok / 0 bad, 0 RS bytes corrected" in r.stderr
    r = _dabmod_file(fin, str(tmp_path / "out"), ["--gpu-frontend", "--superframe", "0"])
    assert r.returncode == 2 and "--superframe does not go without --loopback" in r.stderr
    r = _dabmod_file(fin, str(tmp_path / "out"), opts + ["--superframe", "3"])
    assert r.returncode == 1 and "--superframe: the file has 1 sub-channels" in r.stderr
