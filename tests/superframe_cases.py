"""What the superframe tests share: the reference's Reed-Solomon code behind oracle.ref() (lib/fec: init_rs_char, encode_rs_char,
decode_rs_char, compiled into oracle/_ref/libdabref.so by the committed recipe), seeded error patterns, the classes a decode falls
into, and the golden fixture (tests/golden/superframe_rs.json; tests/golden/make_superframe_rs.py writes it)."""
import ctypes as C
import json
import os

import numpy as np

from tests import superframe_model as SM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "superframe_rs.json")

# positions every error test hits: both ends, both sides of lane 63 / 64 and of the data / parity seam
EDGES = (0, 63, 64, 109, 110, 119)


class Libfec:
    """TS 102 563's code in the reference's library: init_rs_char(8, 0x11d, 0, 1, 10, 135)"""

    def __init__(self):
        import oracle as O
        r = O.ref()
        r.init_rs_char.restype = C.c_void_p
        r.init_rs_char.argtypes = [C.c_int] * 6
        r.encode_rs_char.restype = None
        r.encode_rs_char.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        r.decode_rs_char.restype = C.c_int
        r.decode_rs_char.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int), C.c_int]
        self.r = r
        self.h = r.init_rs_char(8, 0x11D, 0, 1, 10, SM.PAD)
        assert self.h

    def parity(self, data):
        out = C.create_string_buffer(10)
        self.r.encode_rs_char(self.h, bytes(data), out)
        return out.raw

    def decode(self, word):
        """(bytes after the call, return value, locations): locations in the 255-symbol frame, below 135 = padding"""
        buf = C.create_string_buffer(bytes(word), SM.N)
        loc = (C.c_int * 10)()
        n = self.r.decode_rs_char(self.h, buf, loc, 0)
        return buf.raw, n, [int(loc[i]) for i in range(max(n, 0))]


def random_word(rs):
    return SM.rs_encode(bytes(rs.randint(0, 256, SM.K).astype(np.uint8)))


def corrupt(word, rs, n_err, must=()):
    """n_err byte errors at distinct positions, those of `must` first"""
    pos = list(must)[:n_err]
    while len(pos) < n_err:
        p = int(rs.randint(0, SM.N))
        if p not in pos:
            pos.append(p)
    w = bytearray(word)
    for p in pos:
        w[p] ^= int(rs.randint(1, 256))
    return bytes(w)


def classify(ret, loc):
    """refused: libfec returns -1; padding: a location below 135; else: corrected (rightly or to another codeword)"""
    if ret < 0:
        return "refused"
    if any(l < SM.PAD for l in loc):
        return "padding"
    return "corrected"


def check_against_libfec(bad, after, ret, loc, word=None):
    """the model on `bad` against what libfec made of it; returns the class (corrected words that are not `word`: miscorrected)"""
    got, n = SM.rs_decode(bad)
    kind = classify(ret, loc)
    if kind == "corrected":
        assert (got, n) == (after, ret), (bad.hex(), ret, loc, n)
        if word is not None and after != word:
            kind = "miscorrected"
    else:
        assert n == -1 and got == bad, (kind, bad.hex(), ret, loc, n)
    return kind


def golden():
    """the fixture's entries, expanded: word, bad, after (hex), ret, loc"""
    g = json.load(open(GOLDEN))
    out = []
    for e in g["entries"]:
        word = bytes.fromhex(g["words"][e["w"]])
        bad = bytearray(word)
        for p, x in e["err"]:
            bad[p] ^= x
        after = bytearray(bad)
        for p, x in e["fix"]:
            after[p] ^= x
        out.append(dict(word=word.hex(), bad=bytes(bad).hex(), after=bytes(after).hex(), ret=e["ret"], loc=e["loc"], n_err=len(e["err"])))
    return out


# ---- the loop: an ETI stream of 45 frames in Mode II with one 32 kbit/s EEP 3-A sub-channel (s = 4) that carries model superframes
# from frame 2 on; the decoder returns frame i as output i + 15, so 30 images lie behind the lead-in: 26 candidates, superframes
# at 2, 7, 12, 17, 22 (the one from frame 27 on is cut off)
LOOP_MODE, LOOP_FRAMES, LOOP_PHASE, LOOP_EARLY = 2, 45, 2, 44
LOOP_SUBCHANNELS = ((0, 12, 0x22),)
LOOP_S, LOOP_OFFSET, LOOP_FRAMESIZE = 4, 12 + 4 + 96, 96
LOOP_ACCEPTED = [2, 7, 12, 17, 22]
# The noisy point: seeded white noise from the channel emulator, the level by the sweep of tools/time_superframe.py --sweep
# (profiles/superframe.txt): the highest C/N in 0.25 dB steps from 6 dB down at which decode_soft leaves payload bit errors
# behind the lead-in while no RS word needs more than 3 corrections.
LOOP_SEED, LOOP_CN_DB = 4, 4.5


def loop_stream(random_payload=False):
    """(ETI frames, [(first frame, AUs)]): the stream above; random_payload: the sub-channel keeps synth_eti's random bytes"""
    from tests.golden.synth import synth_eti
    eti = synth_eti(LOOP_FRAMES, subchannels=LOOP_SUBCHANNELS, mid=2, seed=4321)
    if random_payload:
        return eti, []
    images, placed = SM.stream_images(LOOP_FRAMES, LOOP_S, LOOP_OFFSET, LOOP_PHASE, 99, fill="zero")
    fs = LOOP_FRAMESIZE
    for f, _ in placed:
        eti[f:f + 5, LOOP_OFFSET:LOOP_OFFSET + fs] = images[f:f + 5, LOOP_OFFSET:LOOP_OFFSET + fs]
    return eti, placed


class Loop:
    """chain_eti -> channel_dev -> demod_soft -> decode_soft_dev -> superframe_dev on one context, device tensors throughout; the
    IQ is made once.  run(cn_db, seed) -> dict(bit_errors, images, out, records, result); cn_db None: no channel."""

    def __init__(self, pkg, eti):
        import torch
        self.pkg, self.eti, self.torch = pkg, eti, torch
        n = self.n = eti.shape[0]
        m = self.m = pkg.Modulator(mode=LOOP_MODE, max_frames=n)
        m.set_gain(2, 1.0, 1.0, 4.0)
        m.set_fir_taps(None)
        m.frontend_configure(eti[0])
        per = m.geometry["tf_input_bytes"]
        d_cod = torch.zeros((n, per), dtype=torch.uint8, device="cuda")
        self.d_iq = torch.zeros(n * m.geometry["tf_samples"], dtype=torch.complex64, device="cuda")
        m.chain_eti_dev_queued(torch.from_numpy(eti).cuda(), n, 3, d_cod, self.d_iq)
        m.synchronize()
        iq = self.d_iq.cpu().numpy().reshape(n, -1)[:, m.geometry["null_size"]:].astype(np.complex128)
        self.power = float(np.mean(np.abs(iq) ** 2))       # mean power behind the null symbol: what dabmod_file --channel-cn takes
        self.d_rx = torch.zeros_like(self.d_iq)
        self.d_soft = torch.zeros((n, 8 * per), dtype=torch.int8, device="cuda")
        ref = np.zeros((n, 6144), np.uint8)
        ref[15:] = eti[:n - 15]
        self.d_ref = torch.from_numpy(ref).cuda()
        self.d_img = torch.zeros(n * 6144, dtype=torch.uint8, device="cuda")
        self.d_out = torch.zeros((n - 15 - 4) * 110 * LOOP_S, dtype=torch.uint8, device="cuda")

    def run(self, cn_db=None, seed=0):
        m, n = self.m, self.n
        m.decode_reset()
        src = self.d_iq
        if cn_db is not None:
            m.set_channel([(0, 1.0, 0.0)], self.pkg.channel_sigma(self.power, cn_db), seed)
            m.channel_reset(0)
            m.channel_dev(self.d_iq, self.d_rx)
            src = self.d_rx
        m.demod_soft_dev(src, n, self.d_soft, LOOP_EARLY)
        m.decode_soft_dev(self.d_soft, n, self.d_img, self.d_ref)
        m.superframe_dev(self.d_img[15 * 6144:], n - 15, LOOP_OFFSET, LOOP_FRAMESIZE, self.d_out)
        self.torch.cuda.synchronize()
        unit = [m.decode_soft_stats(i, 1) for i in range(15, n)]
        return dict(bit_errors=sum(u["bit_errors"] for u in unit), images=self.d_img.cpu().numpy().reshape(n, 6144)[15:],
                    out=self.d_out.cpu().numpy(), records=m.superframe_records(), result=m.superframe_result())

    def close(self):
        self.m.close()


def golden_subchannel(entries, s=8):
    """the fixture's corrupted words laid out as sub-channel frames of s = 8: groups of s words -> ([120 s bytes], entries per group)"""
    groups = []
    for g in range(0, len(entries) - len(entries) % s, s):
        part = entries[g:g + s]
        buf = bytearray(SM.N * s)
        for i, e in enumerate(part):
            buf[i::s] = bytes.fromhex(e["bad"])
        groups.append((bytes(buf), part))
    return groups
