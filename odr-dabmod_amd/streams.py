"""Multi-GPU harness: one process per GPU, each modulating its own independent
stream of transmission frames (frames are independent units, so the
path shards with NO data-path collective) -- or, with partition_chunks / my_chunks /
PartitionedStream, its share of ONE stream, whose state in front of a chunk follows
from the one frame before it (from the ETI frames eti_leadin names, where the front-end
runs on the device too).  torch.distributed (backend "nccl" =
RCCL on ROCm, "gloo" in CPU tests) is used only to bracket the timed region and
to combine the ranks' clocks."""
import os
import sys
import time

import numpy as np


def partition_chunks(n_frames, chunk, parts):
    """ONE stream of n_frames transmission frames cut into chunks of `chunk` frames (the last may be short), chunk j going
    to part j mod parts: per part the list of (start, stop) it modulates, in stream order.  The owner of a chunk needs no
    other part's result: its stream state in front of frame `start` follows from frame start - 1 alone (the lead-in frame
    of Modulator.seed; none for start == 0)."""
    n_frames, chunk, parts = int(n_frames), int(chunk), int(parts)
    if n_frames < 0 or chunk < 1 or parts < 1:
        raise ValueError("partition_chunks: n_frames >= 0, chunk >= 1, parts >= 1")
    out = [[] for _ in range(parts)]
    for j, start in enumerate(range(0, n_frames, chunk)):
        out[j % parts].append((start, min(start + chunk, n_frames)))
    return out


def eti_leadin(e, cifs, with_chain=True):
    """The ETI frames a context reads to take a stream up at ETI frame `e` (a multiple of cifs, the frames per
    transmission frame): (start, stop) with stop = e.  The time interleaver looks fifteen frames back (Modulator.frontend_seed);
    with the chain behind it the transmission frame in front of e is needed whole, and the fifteen frames in front of THAT
    one (Modulator.seed_eti).  Shorter where the stream starts."""
    e, cifs = int(e), int(cifs)
    if e < 0 or cifs < 1 or e % cifs:
        raise ValueError("eti_leadin: e >= 0, a multiple of cifs >= 1")
    return max(0, e - (15 + (cifs if with_chain else 0))), e


class PartitionedStream:
    """One stream split over several contexts (on one GPU or on several): chunk j of the stream goes to context j mod N,
    which first computes its own starting state from the chunk's lead-in frame (Modulator.seed_dev) and so waits for no
    other context.  All contexts must have been given the same settings by the caller.  Every context runs on one lane (a
    chain call with the Resampler uses lane 0 only, and so does the seed in front of it); contexts in one process share the
    runtime's hardware queues, whose number is the process's to choose."""

    def __init__(self, modulators):
        self.mods = list(modulators)
        if not self.mods:
            raise ValueError("PartitionedStream: at least one context")
        for md in self.mods:
            md.set_lanes(1)

    def modulate(self, bits, stages, chunk, out=None):
        """bits: n_frames x tf_input_bytes coded bits of consecutive frames, frame 0 the start of the stream -- a numpy
        array, or a torch uint8 tensor on the GPU (then `out`, if given, is the device tensor to fill, and the result is
        one).  Queues every seed and every chunk before it waits for anything; returns the frames in stream order, the
        bytes one context gives for the whole stream."""
        import torch
        md0 = self.mods[0]
        per = md0.geometry["tf_input_bytes"]
        host = not isinstance(bits, torch.Tensor)
        dev = torch.device("cuda", md0.device)
        d_bits = (torch.from_numpy(np.ascontiguousarray(bits, np.uint8).reshape(-1, per)).to(dev) if host
                  else bits.reshape(-1, per))
        n = d_bits.shape[0]
        dt = np.dtype(getattr(md0, "_out_dtype", np.complex64))
        per_out = md0.out_bytes_per_frame(stages) // dt.itemsize
        tdt = {"complex64": torch.complex64, "int16": torch.int16, "uint8": torch.uint8, "int8": torch.int8}[dt.name]
        d_out = out if (out is not None and not host) else torch.empty((n, per_out), dtype=tdt, device=dev)
        if d_out.numel() != n * per_out or d_out.dtype != tdt or not d_out.is_contiguous():
            raise ValueError("PartitionedStream: output tensor does not match (%s, %d elements, contiguous)" % (tdt, n * per_out))
        d_out = d_out.reshape(n, per_out)
        torch.cuda.current_stream(dev).synchronize()          # (the input is in place before any context reads it)
        chunks = sorted((c, i) for i, part in enumerate(partition_chunks(n, chunk, len(self.mods))) for c in part)
        for (start, stop), i in chunks:
            md = self.mods[i]
            md.seed_dev(d_bits[start - 1] if start else None, stages, start, queued=True)
            md.chain_dev_queued(d_bits[start:stop], stop - start, stages, d_out[start:stop])
        for md in self.mods:
            md.synchronize()
        if not host:
            return d_out
        res = d_out.cpu().numpy()
        if out is not None:
            np.copyto(out.reshape(res.shape), res)
            return out.reshape(res.shape)
        return res


    def modulate_eti(self, eti, stages, chunk, out=None):
        """modulate() from raw ETI frames: eti is n x 6144 bytes of consecutive frames, frame 0 the start of the stream (FP =
        0), whole transmission frames -- a numpy array or a torch uint8 tensor on the GPU; `chunk` counts transmission
        frames.  Every context has been configured from eti[0] by the caller (Modulator.frontend_configure).  Chunk j goes
        to context j mod N, which first seeds front-end and chain from the frames in front of the chunk (eti_leadin,
        Modulator.seed_eti_dev) and then runs the chunk from the device's copy of the frames; the coded bits never leave
        the device.  Returns the bytes one context's chain_eti gives for the whole stream."""
        import torch
        md0 = self.mods[0]
        cifs = {1: 4, 2: 1, 3: 1, 4: 2}[md0.geometry["mode"]]
        per = md0.geometry["tf_input_bytes"]
        host = not isinstance(eti, torch.Tensor)
        dev = torch.device("cuda", md0.device)
        d_eti = (torch.from_numpy(np.ascontiguousarray(eti, np.uint8).reshape(-1, 6144)).to(dev) if host
                 else eti.reshape(-1, 6144))
        if d_eti.shape[0] % cifs:
            raise ValueError("PartitionedStream: ETI frames come as whole transmission frames (a multiple of %d)" % cifs)
        n = d_eti.shape[0] // cifs
        dt = np.dtype(getattr(md0, "_out_dtype", np.complex64))
        per_out = md0.out_bytes_per_frame(stages) // dt.itemsize
        tdt = {"complex64": torch.complex64, "int16": torch.int16, "uint8": torch.uint8, "int8": torch.int8}[dt.name]
        d_out = out if (out is not None and not host) else torch.empty((n, per_out), dtype=tdt, device=dev)
        if d_out.numel() != n * per_out or d_out.dtype != tdt or not d_out.is_contiguous():
            raise ValueError("PartitionedStream: output tensor does not match (%s, %d elements, contiguous)" % (tdt, n * per_out))
        d_out = d_out.reshape(n, per_out)
        # the coded bits of a chunk: scratch per context (a context's calls run in order)
        d_bits = [torch.empty((min(int(chunk), max(n, 1)), per), dtype=torch.uint8, device=dev) for _ in self.mods]
        torch.cuda.current_stream(dev).synchronize()          # (the input is in place before any context reads it)
        chunks = sorted((c, i) for i, part in enumerate(partition_chunks(n, chunk, len(self.mods))) for c in part)
        for (start, stop), i in chunks:
            md = self.mods[i]
            a, e = eti_leadin(start * cifs, cifs)
            md.seed_eti_dev(d_eti[a:e] if e > a else None, e - a, stages, e, queued=True)
            md.chain_eti_dev_queued(d_eti[e:stop * cifs], (stop - start) * cifs, stages, d_bits[i][:stop - start],
                                    d_out[start:stop])
        for md in self.mods:
            md.synchronize()
        if not host:
            return d_out
        res = d_out.cpu().numpy()
        if out is not None:
            np.copyto(out.reshape(res.shape), res)
            return out.reshape(res.shape)
        return res


class StreamGroup:
    def __init__(self, backend=None, device_index=None):
        import torch
        import torch.distributed as dist
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        # the GPU this rank drives (default: its local rank)
        self.device_index = self.local_rank if device_index is None else int(device_index)
        self._dist = dist
        self._torch = torch
        self.backend = backend
        # DABGPU_FORCE_DIST=1 initialises the process group for a single rank too (exercises the RCCL path
        # on a one-GPU box)
        self._collective = self.world > 1 or os.environ.get("DABGPU_FORCE_DIST") == "1"
        if self._collective and not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            backend = backend or ("nccl" if torch.cuda.is_available() else "gloo")
            self.backend = backend
            kw = {}
            if backend == "nccl":
                kw["device_id"] = torch.device("cuda", self.device_index)
            # RCCL prints its version banner on the C-level stdout whenever it first creates a communicator -- at
            # init, at the first collective of a kind, or as late as teardown.  The bench's stdout carries exactly
            # one JSON line, so for the life of the group file descriptor 1 points at stderr and the line goes out
            # through a private duplicate of the real stdout (emit()).
            sys.stdout.flush()
            self._out_fd = os.dup(1)
            os.dup2(2, 1)
            dist.init_process_group(backend, **kw)
            dist.barrier()

    def emit(self, text):
        """Write one line to the process's real stdout (see __init__)."""
        fd = getattr(self, "_out_fd", None)
        if fd is None:
            print(text, flush=True)
        else:
            os.write(fd, (text + "\n").encode())

    def barrier(self):
        if self._collective:
            self._dist.barrier()

    def max_over_ranks(self, seconds):
        """The job's elapsed time is the slowest rank's."""
        if not self._collective:
            return float(seconds)
        dev = "cuda:%d" % self.device_index if self.backend == "nccl" else "cpu"
        t = self._torch.tensor([float(seconds)], dtype=self._torch.float64, device=dev)
        self._dist.all_reduce(t, op=self._dist.ReduceOp.MAX)
        return float(t.item())

    def min_over_ranks(self, value):
        """The smallest of the ranks' integers (the batch every rank can hold: weak scaling keeps per-GPU work equal)."""
        if not self._collective:
            return int(value)
        dev = "cuda:%d" % self.device_index if self.backend == "nccl" else "cpu"
        t = self._torch.tensor([int(value)], dtype=self._torch.int64, device=dev)
        self._dist.all_reduce(t, op=self._dist.ReduceOp.MIN)
        return int(t.item())

    def my_chunks(self, n_frames, chunk):
        """This rank's chunks of ONE stream split over the ranks (partition_chunks over rank and world size): each rank
        seeds its context from frame start - 1 and modulates [start, stop) without hearing from the others."""
        return partition_chunks(n_frames, chunk, self.world)[self.rank]

    def stream_seed(self, base=42):
        """Every rank modulates a different stream (different synthetic input)."""
        return base + self.rank

    def timed(self, fn, steps, sync):
        """barrier + device sync, `steps` calls of fn, device sync + barrier; MAX over ranks."""
        self.barrier()
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        sync()
        self.barrier()
        return self.max_over_ranks(time.perf_counter() - t0)

    def job_frames_per_second(self, frames_per_step_per_gpu, steps, seconds):
        """Whole-job throughput: every rank processed frames_per_step_per_gpu * steps frames."""
        return self.world * frames_per_step_per_gpu * steps / seconds

    def gather_to_root(self, t, root=0):
        """OPTIONAL final gather of the ranks' IQ (north_star: "RCCL over xGMI only for an optional
        final IQ gather"): every rank's tensor `t` lands on `root`, in rank order.  Never on the modulation path --
        frames are independent and each stream's sink may just as well sit behind its own GPU.  Over xGMI every
        non-root rank owns one point-to-point link to the root (~153 GB/s each way), so the root receives
        (N - 1) * t.nbytes over N - 1 links in parallel: the gather is bound per link by t.nbytes / 153 GB/s, and
        on the root by its HBM write rate only.  Returns the list of N tensors on the root, None elsewhere."""
        torch, dist = self._torch, self._dist
        if not self._collective:
            return [t]
        cplx = t.is_complex()
        if cplx:
            t = torch.view_as_real(t)            # (RCCL has no complex element type: the same bytes as float pairs)
        dev = t.device
        if self.backend == "gloo" and dev.type != "cpu":
            t = t.cpu()                          # (gloo gathers host tensors only: ranks that share a GPU in the tests)
        out = [torch.empty_like(t) for _ in range(self.world)] if self.rank == root else None
        dist.gather(t.contiguous(), out, dst=root)
        if out is not None and out[0].device != dev:
            out = [o.to(dev) for o in out]
        if out is not None and cplx:
            out = [torch.view_as_complex(o) for o in out]
        return out

    def close(self):
        if self._collective and self._dist.is_initialized():
            self._dist.destroy_process_group()
        # (fd 1 stays on stderr until the process exits: RCCL may still print while it unloads)
