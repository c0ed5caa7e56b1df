"""The stream state in the C-ABI, the parts that need no GPU: the five entry points are declared and exported, the partition
of one stream into chunks is exact, two ranks' shares of it are disjoint and complete, and dabmod_file refuses a --contexts
it cannot honour before any context exists."""
import itertools
import os
import socket
import subprocess
import sys
import textwrap

import pytest

from tests.conftest import ROOT, load_pkg

HOST = os.path.join(ROOT, "odr-dabmod_amd", "host")
NAMES = ("dabgpu_stream_state_bytes", "dabgpu_get_stream_state", "dabgpu_set_stream_state", "dabgpu_chain_seed",
         "dabgpu_chain_seed_dev")


def test_header_declares_and_library_exports_the_stream_state_entry_points():
    import re
    pkg = load_pkg()
    pkg.build()
    text = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    declared = set(re.findall(r"DABGPU_API[^;]*?\b(dabgpu_[a-z_0-9]+)\s*\(", text, re.S))
    lib = pkg.load_library()
    for name in NAMES:
        assert name in declared, name
        assert name in pkg.EXPORTS, name
        assert hasattr(lib, name), "libdabgpu.so does not export %s" % name
    # the comments name the reference's own state: the Resampler's input window and TII::m_insert
    i = text.index("stream state: one resampled stream")
    comment = text[i:text.index("DABGPU_API size_t dabgpu_stream_state_bytes")]
    assert "src/Resampler.cpp:142-147" in comment and ":188-191" in comment and "src/TII.cpp:226-242" in comment
    # the documented layout is the one the library is compiled with (a static_assert holds the other end)
    assert "DABGPU_STREAM_STATE_HEADER_BYTES 40" in text


def streams_module():
    import importlib
    load_pkg()
    return importlib.import_module("odr-dabmod_amd.streams")


@pytest.mark.parametrize("parts", [1, 2, 3, 4])
@pytest.mark.parametrize("chunk", [1, 2, 5, 16])
@pytest.mark.parametrize("n_frames", [0, 1, 3, 12, 16, 17, 33])
def test_partition_chunks_covers_the_stream_exactly_once_in_order(n_frames, chunk, parts):
    """Chunk j = frames [j chunk, min((j + 1) chunk, n)) goes to part j mod parts; every part's list is in stream order; the
    union is range(n_frames) with nothing twice; only the last chunk may be short; the lead-in frame of a chunk is the frame
    before its first (none for the chunk that starts the stream).  The grid has n_frames < chunk, ragged tails and parts = 1."""
    st = streams_module()
    per_part = st.partition_chunks(n_frames, chunk, parts)
    assert len(per_part) == parts
    flat = sorted(itertools.chain.from_iterable(per_part))
    assert [f for a, b in flat for f in range(a, b)] == list(range(n_frames))
    for j, (a, b) in enumerate(flat):
        assert a == j * chunk and 0 < b - a <= chunk and (b - a == chunk or b == n_frames)
        assert (a, b) in per_part[j % parts]
        leadin = a - 1
        assert leadin == (-1 if j == 0 else flat[j - 1][1] - 1)
    for part in per_part:
        assert part == sorted(part)
    if parts == 1:
        assert per_part[0] == flat


def test_partition_chunks_refuses_nonsense():
    st = streams_module()
    for bad in ((-1, 4, 2), (8, 0, 2), (8, 4, 0)):
        with pytest.raises(ValueError):
            st.partition_chunks(*bad)


WORKER = textwrap.dedent("""
    import importlib, json, sys
    sys.path.insert(0, %r)
    streams = importlib.import_module("odr-dabmod_amd.streams")
    g = streams.StreamGroup(backend="gloo")
    assert g.world == 2
    mine = g.my_chunks(23, 4)
    assert mine == streams.partition_chunks(23, 4, 2)[g.rank]
    g.barrier()
    g.emit(json.dumps({"rank": g.rank, "chunks": mine}))
    g.close()
""") % ROOT


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_take_disjoint_and_complete_shares_of_one_stream(tmp_path):
    """Two processes over gloo (the pattern of tests/test_streams_gloo.py): StreamGroup.my_chunks gives each rank its chunks
    of ONE stream of 23 frames in chunks of 4 -- disjoint, together every frame once, alternating in stream order."""
    import json
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    port = free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                      text=True))
    outs = []
    for p in procs:
        o, e = p.communicate(timeout=120)
        assert p.returncode == 0, e[-2000:]
        outs.append(json.loads(o.strip().splitlines()[-1]))
    outs.sort(key=lambda d: d["rank"])
    a, b = ([tuple(c) for c in d["chunks"]] for d in outs)
    assert not set(a) & set(b)
    frames = sorted(f for s, t in a + b for f in range(s, t))
    assert frames == list(range(23))
    order = sorted((c, r) for r, cs in enumerate((a, b)) for c in cs)
    assert [r for _, r in order] == [0, 1, 0, 1, 0, 1]
    assert order[-1][0] == (20, 23)


@pytest.mark.parametrize("args", [["--contexts", "2"], ["--batch", "1", "--contexts", "2"], ["--batch", "4", "--contexts", "0"],
                                  ["--batch", "4", "--contexts", "5"], ["--batch", "4", "--contexts"],
                                  ["--batch", "4", "--contexts", "2x"], ["--batch", "4", "--contexts", "2", "--bits-only"],
                                  ["--batch", "4", "--contexts", "2", "--separate-converter"]])
def test_dabmod_file_refuses_contexts_it_cannot_honour(tmp_path, args):
    """--contexts N splits the BATCHES of the streaming path: without --batch B > 1, or outside 1 ... 4, it is a usage error
    -- exit status 2 and the usage text, before the input is opened or any context exists (no GPU is involved)."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "odr-dabmod_amd", "csrc"), "-j2"])
    subprocess.check_call(["make", "-s", "-C", HOST, "-j2"])
    fin, fout = str(tmp_path / "missing.eti"), str(tmp_path / "out.iq")
    r = subprocess.run([os.path.join(HOST, "dabmod_file"), fin, fout] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert r.stderr.startswith("usage: dabmod_file") and "--contexts N" in r.stderr
    assert not os.path.exists(fout)
