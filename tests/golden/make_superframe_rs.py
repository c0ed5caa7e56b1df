"""Writes tests/golden/superframe_rs.json: what the reference's Reed-Solomon decoder (lib/fec behind oracle.ref(), set up as TS 102 563's
RS(120,110)) makes of about 200 corrupted words, so that tests/test_superframe_cpu.py can hold the model to it where the reference
is absent.  Data only: 16 codewords, and per entry the word's index, the errors put in [(position, xor)], decode_rs_char's return
value, the locations it reported (in the 255-symbol frame: below 135 is padding) and the changes it made [(position, xor)].
Classes: 1 ... 5 errors (corrected), 6 ... 12 errors refused, with a root in the padding, and miscorrected to another codeword.

    python tests/golden/make_superframe_rs.py          (needs oracle/_ref/libdabref.so)
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import superframe_cases as SC                  # noqa: E402
from tests import superframe_model as SM                  # noqa: E402


def main():
    fec = SC.Libfec()
    rs = np.random.RandomState(102563)
    words = []
    for _ in range(16):
        data = bytes(rs.randint(0, 256, SM.K).astype(np.uint8))
        words.append(data + fec.parity(data))
    entries = []

    def attempt(w, n_err, must=()):
        pos = list(must)[:n_err]
        while len(pos) < n_err:
            p = int(rs.randint(0, SM.N))
            if p not in pos:
                pos.append(p)
        err = [[p, int(rs.randint(1, 256))] for p in pos]
        bad = bytearray(words[w])
        for p, x in err:
            bad[p] ^= x
        after, ret, loc = fec.decode(bytes(bad))
        fix = [[p, bad[p] ^ after[p]] for p in range(SM.N) if bad[p] != after[p]]
        kind = SC.classify(ret, loc)
        if kind == "corrected" and after != words[w]:
            kind = "miscorrected"
        return dict(w=w, err=err, ret=ret, loc=loc, fix=fix), kind

    for n_err in range(1, 6):                             # 5 x 20 corrected, the edge positions in the first of each count
        for k in range(20):
            e, kind = attempt(k % 16, n_err, SC.EDGES[:n_err] if k == 0 else SC.EDGES[-n_err:] if k == 1 else ())
            assert kind == "corrected" and e["ret"] == n_err
            entries.append(e)
    want = {"refused": 60, "padding": 30, "miscorrected": 6}
    have = dict.fromkeys(want, 0)
    tries = 0
    while any(have[k] < want[k] for k in want):
        tries += 1
        e, kind = attempt(tries % 16, 6 + tries % 7)
        if kind in have and have[kind] < want[kind]:
            have[kind] += 1
            entries.append(e)
    print("%d entries after %d tries beyond t: %s" % (len(entries), tries, have))
    path = SC.GOLDEN
    with open(path, "w") as f:
        json.dump({"words": [w.hex() for w in words], "entries": entries}, f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
