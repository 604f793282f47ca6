"""Cases and byte-exact NumPy model of the stream-ordered IPC exchange
(gmt_ipc_plan_init / gmt_ipc_exchange), shared by tests/test_ipc_gpu.py (the
gfx950 kernel of csrc/kernels/ipc.hip, in-process) and tests/test_ipc_cpu.py
(the CPU backend: this file run as a program in a child process, because
build/lib-host/libgmt.so shares its SONAME with the GPU library).

One process plays both ends of every message, wired like the transport's self
messages (csrc/comm/transport_ipc.cpp, m.peer == rank_): send channel i copies
its source into slot e & 1 of stage[i], waits on cflag[i] and signals rflag[i];
the receive channel that reads stage[i] waits on rflag[i] and signals
cflag[i].  Every wait is satisfied by the launch itself, by an earlier launch
of the same stream, or by a flag the host wrote before the launch (the
single-role plans and the channels without a partner), so nothing can stall.

Everything the kernel may touch lies in ONE device allocation (the arena):
sources, the two parity slots of every stage, destinations, each with 64 guard
bytes or more on either side (the slots of a stage are adjacent, slot 1 at
max(bytes, 1) as in the transport: a byte past one slot lands in the other
one, which is compared as well).  The model holds the same arena as a uint8 array and applies every
exchange to it; after each exchange the whole arena, every flag, the epoch,
the role counters and the error word are compared bitwise, so a byte written
outside a run, into a guard or into the other parity slot shows as the first
differing offset, reported with its channel.  Sources are refilled before
each exchange with bytes that encode (exchange, channel, offset): a stale slot
or a stale source cannot pass.

All memory comes from gmt_rt_malloc, so the same code drives the GPU library
and the CPU backend."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gpu_mpi_tests_amd import _native as nat  # noqa: E402

D = 8              # bytes per double
CHUNK = 16 * 1024  # ipc.hip kBlockBytes
GUARD = 64
EXCHANGES = 6      # both parities three times; exchanges 3.. reach the e - 2 wait
NAMES = ("gmt_rt_backend", "gmt_rt_malloc", "gmt_rt_free", "gmt_rt_memcpy", "gmt_rt_memset_async",
         "gmt_rt_stream_create", "gmt_rt_stream_destroy", "gmt_rt_stream_synchronize", "gmt_rt_stream_begin_capture",
         "gmt_rt_stream_end_capture", "gmt_rt_graph_launch", "gmt_rt_graph_destroy", "gmt_ipc_table_bytes",
         "gmt_ipc_plan_init", "gmt_ipc_exchange", "gmt_slices_reduce", "gmt_stage_copy", "gmt_stage_scatter",
         "gmt_signal_wait", "gmt_fill_poly", "gmt_error_string")


class Rt:
    """gmt_rt memory and one stream of a loaded libgmt.so (either backend)."""

    def __init__(self, lib):
        self.L = nat.bind(lib, NAMES)
        self.hip = self.L.gmt_rt_backend() == 1
        self.allocs = []
        s = ctypes.c_void_p()
        self.ok(self.L.gmt_rt_stream_create(ctypes.byref(s), 0), "stream create")
        self.stream = s

    def ok(self, rc, what):
        if rc != 0:
            msg = self.L.gmt_error_string(rc)
            raise RuntimeError(f"{what}: error {rc} ({msg.decode() if msg else '?'})")

    def malloc(self, nbytes, space):
        p = ctypes.c_void_p()
        self.ok(self.L.gmt_rt_malloc(ctypes.byref(p), nbytes, space), f"malloc {nbytes} in space {space}")
        self.allocs.append((p.value, space))
        return p.value

    def put(self, addr, arr):
        arr = np.ascontiguousarray(arr)
        if arr.nbytes:
            self.ok(self.L.gmt_rt_memcpy(addr, arr.ctypes.data, arr.nbytes), "upload")

    def get(self, addr, count, dtype=np.uint8):
        out = np.zeros(count, dtype)
        if out.nbytes:
            self.ok(self.L.gmt_rt_memcpy(out.ctypes.data, addr, out.nbytes), "download")
        return out

    def sync(self):
        self.ok(self.L.gmt_rt_stream_synchronize(self.stream), "stream synchronize")

    def free_all(self):
        self.L.gmt_rt_stream_synchronize(self.stream)
        for addr, space in reversed(self.allocs):
            self.L.gmt_rt_free(addr, space)
        self.allocs = []

    def close(self):
        self.free_all()
        self.L.gmt_rt_stream_destroy(self.stream)


# ------------------------------------------------------------------ the cases
def S(nbytes, off=0, run=0, ld=0, wait=True, signal=True):
    """A send channel: `nbytes` from a source placed `off` bytes past a 256-byte
    boundary, contiguous or runs of `run` bytes `ld` bytes apart."""
    return dict(bytes=nbytes, off=off, run=run, ld=ld, wait=wait, signal=signal)


def R(nbytes, frm, off=0, run=0, ld=0, wait=True, signal=True):
    """A receive channel reading stage[frm], or (frm None) a stage of its own
    that the host fills before each launch, the host playing the sender."""
    return dict(bytes=nbytes, frm=frm, off=off, run=run, ld=ld, wait=wait, signal=signal)


def pair(nbytes, src=None, dst=None, off=0):
    return ([S(nbytes, off, *(src or (0, 0)))], [R(nbytes, 0, 0, *(dst or (0, 0)))])


def face(run_d, ld_d, runs):
    return run_d * D * runs, (run_d * D, ld_d * D)


def _cases():
    cases = []

    def add(name, sends, recvs, graph=False):
        cases.append(dict(name=name, sends=sends, recvs=recvs, graph=graph))

    # contiguous, one channel: 2049 d makes slot 1 misaligned (the path alternates with the epoch)
    for label, n in (("1d", D), ("2d", 2 * D), ("16K-8", CHUNK - 8), ("16K", CHUNK), ("16K+16", CHUNK + 16),
                     ("2049d", 2049 * D), ("3B", 3)):
        add("contig_" + label, *pair(n))
    add("contig_4097B_src+1", *pair(4097, off=1))
    # a strided face on the send side (in-place W / E face), then on the receive side:
    # vector path one run per lane | byte path | pitch no multiple of 16 B | ld == run
    faces = (("2d_40d_300", face(2, 40, 300)), ("3d_40d_301", face(3, 40, 301)), ("20d_37d_130", face(20, 37, 130)),
             ("2d_2d_1025", face(2, 2, 1025)))
    for label, (n, rl) in faces:
        add("src_face_" + label, *pair(n, src=rl))
    for label, (n, rl) in faces:
        add("dst_face_" + label, *pair(n, dst=rl))
    # 8 + 8 channels: mixed sizes, a zero-byte channel in the middle, one of 3 chunks, a pair without the
    # "consumed" flag (send.wait == NULL, recv.signal == NULL), a send without signal and a receive without
    # wait (each other's stand-ins: that receive reads a stage the host wrote)
    n6, rl6 = face(2, 5, 7)
    add("table_8+8",
        [S(24), S(2 * CHUNK + 4000), S(4096), S(0), S(1000, wait=False), S(520, signal=False), S(n6, 0, *rl6),
         S(CHUNK)],
        [R(24, 0), R(2 * CHUNK + 4000, 1), R(4096, 2), R(0, 3), R(1000, 4, signal=False), R(48, None, wait=False),
         R(n6, 6), R(CHUNK, 7, 0, 4 * D, 5 * D)])
    # more than 128 chunks per role: the grid-stride walk changes channel in mid-walk
    big = [130 * CHUNK + 24, D, 5 * CHUNK]
    add("over_128_chunks", [S(n) for n in big], [R(n, i) for i, n in enumerate(big)])
    # single-role plans: the host plays the other role through the flags (and the slots)
    n9, rl9 = face(2, 6, 9)
    add("send_only", [S(CHUNK + 16), S(24), S(0), S(n9, 0, *rl9)], [])
    n11, rl11 = face(3, 7, 11)
    add("recv_only", [], [R(CHUNK + 16, None), R(40, None), R(0, None), R(n11, None, 0, *rl11)])
    # one captured exchange replayed 4 times with eager launches in between
    n3, rl3 = face(2, 40, 300)
    add("graph_replay", [S(2049 * D), S(n3, 0, *rl3), S(3)], [R(2049 * D, 0), R(n3, 1), R(3, 2, 0)], graph=True)
    return cases


CASES = _cases()
CASE_NAMES = [c["name"] for c in CASES]
GRAPH_TURNS = ("eager", "graph", "graph", "eager", "graph", "eager", "graph")


# ------------------------------------------------------------------ the model
def pattern(e, chan, n):
    """n bytes that encode (exchange, channel, offset)."""
    o = np.arange(n, dtype=np.int64)
    return ((o * 131 + (o >> 8) * 29 + (o >> 16) * 7 + e * 97 + chan * 53 + 17) & 0xFF).astype(np.uint8)


def extent(c):
    """Bytes a channel's (possibly strided) side spans."""
    if c["run"] == 0 or c["bytes"] == 0:
        return c["bytes"]
    return (c["bytes"] // c["run"] - 1) * c["ld"] + c["run"]


def byte_map(c):
    """Offset within the side's buffer of every message byte (the kernel's at())."""
    o = np.arange(c["bytes"], dtype=np.int64)
    if c["run"] == 0:
        return o
    return o // c["run"] * c["ld"] + o % c["run"]


class Layout:
    """Regions of the arena: payload at 256 B + off, at least GUARD bytes of guard on either side."""

    def __init__(self):
        self.regions = []  # (start, size, name)
        self.cursor = 0

    def add(self, name, size, off=0):
        start = (self.cursor + GUARD + 255) // 256 * 256 + off
        self.regions.append((start, size, name))
        self.cursor = start + size + GUARD
        return start

    def total(self):
        return self.cursor + GUARD

    def describe(self, offset):
        for start, size, name in self.regions:
            if start <= offset < start + size:
                return f"{name} byte offset {offset - start}"
        after = [r for r in self.regions if r[0] + r[1] <= offset]
        if after:
            start, size, name = max(after)
            return f"guard, {offset - start - size} bytes past the end of {name}"
        return f"guard, {self.regions[0][0] - offset} bytes before {self.regions[0][2]}"


def run_case(rt, case, log=None):
    """Runs one case on rt's library; raises AssertionError naming the channel and byte offset."""
    L = rt.L
    sends, recvs = case["sends"], case["recvs"]
    ns, nr = len(sends), len(recvs)
    name = case["name"]
    for j, r in enumerate(recvs):  # a receive may only read what is complete before it reads
        if r["frm"] is None:
            continue
        assert r["wait"] and sends[r["frm"]]["signal"] and sends[r["frm"]]["bytes"] == r["bytes"], (name, j)
    lay = Layout()
    src = [lay.add(f"send channel {i} source", extent(c), c["off"]) for i, c in enumerate(sends)]
    stride = [max(c["bytes"], 1) for c in sends]
    stage = [lay.add(f"send channel {i} stage (slot 1 at byte {stride[i]})", 2 * stride[i]) for i in range(ns)]
    ostride = [max(c["bytes"], 1) for c in recvs]
    ostage = [lay.add(f"receive channel {j} host-written stage (slot 1 at byte {ostride[j]})", 2 * ostride[j])
              if c["frm"] is None else None for j, c in enumerate(recvs)]
    dst = [lay.add(f"receive channel {j} destination", extent(c), c["off"]) for j, c in enumerate(recvs)]
    size = lay.total()
    model = ((np.arange(size, dtype=np.int64) * 37 + 11) & 0xFF).astype(np.uint8)
    # flags: rflag[i] | cflag[i] of the sends, then ready | consumed of the receives with a stage of their own
    nflags = 2 * ns + 2 * nr
    rflag = lambda i: i                 # noqa: E731
    cflag = lambda i: ns + i            # noqa: E731
    orflag = lambda j: 2 * ns + j       # noqa: E731
    ocflag = lambda j: 2 * ns + nr + j  # noqa: E731
    try:
        arena = rt.malloc(size, nat.SPACE_DEVICE)
        flags = rt.malloc(8 * nflags, nat.SPACE_FLAGS)
        ctl = rt.malloc(32, nat.SPACE_DEVICE)  # epoch | counters[3]
        table = rt.malloc(int(L.gmt_ipc_table_bytes(ns + nr)), nat.SPACE_DEVICE)
        err = rt.malloc(4, nat.SPACE_PINNED)
        mflags = np.zeros(nflags, np.uint64)
        rt.put(arena, model)
        rt.put(flags, mflags)
        rt.put(ctl, np.zeros(32, np.uint8))
        rt.put(err, np.zeros(4, np.uint8))

        fl = lambda k: flags + 8 * k  # noqa: E731
        send_c = (nat.IpcChan * max(ns, 1))()
        recv_c = (nat.IpcChan * max(nr, 1))()
        host_cflag = []  # sends whose "consumed" flag nobody in the plan raises: the host does
        for i, c in enumerate(sends):
            send_c[i] = nat.IpcChan(arena + src[i], arena + stage[i], c["bytes"], 0, stride[i],
                                    fl(cflag(i)) if c["wait"] else None, fl(rflag(i)) if c["signal"] else None,
                                    c["run"], c["ld"], 0, 0)
            if c["wait"] and not any(r["frm"] == i and r["signal"] for r in recvs):
                host_cflag.append(i)
        for j, c in enumerate(recvs):
            own = c["frm"] is None
            base, st = (ostage[j], ostride[j]) if own else (stage[c["frm"]], stride[c["frm"]])
            wait = fl(orflag(j) if own else rflag(c["frm"])) if c["wait"] else None
            signal = fl(ocflag(j) if own else cflag(c["frm"])) if c["signal"] else None
            recv_c[j] = nat.IpcChan(arena + base, arena + dst[j], c["bytes"], st, 0, wait, signal, 0, 0, c["run"],
                                    c["ld"])
        plan = nat.IpcPlan(table, ctl, ctl + 8, err, 0, 0, 0, 0)
        rt.ok(L.gmt_ipc_plan_init(ctypes.byref(plan), ns, send_c if ns else None, nr, recv_c if nr else None),
              f"{name}: gmt_ipc_plan_init")
        chunks = lambda cs: sum(max(1, -(-c["bytes"] // CHUNK)) for c in cs)  # noqa: E731
        if rt.hip:  # a zero-byte channel still takes one chunk
            got = (plan.n_send, plan.n_recv, plan.send_chunks, plan.recv_chunks)
            assert got == (ns, nr, chunks(sends), chunks(recvs)), (name, got)

        def compare(e, what):
            got = rt.get(arena, size)
            if not np.array_equal(got, model):
                o = int(np.flatnonzero(got != model)[0])
                raise AssertionError(f"{name}, {what}: {lay.describe(o)}: got {int(got[o])}, expected {int(model[o])} "
                                     f"({int((got != model).sum())} bytes differ)")
            gf = rt.get(flags, nflags, np.uint64)
            assert gf.tolist() == mflags.tolist(), f"{name}, {what}: flags {gf.tolist()}, expected {mflags.tolist()}"
            c = rt.get(ctl, 8, np.uint32)
            state = (int(c[0]) | int(c[1]) << 32, c[2:5].tolist(), int(rt.get(err, 1, np.uint32)[0]))
            assert state == (e, [0, 0, 0], 0), f"{name}, {what}: (epoch, counters, err) = {state}, expected epoch {e}"

        graph = ctypes.c_void_p()
        turns = GRAPH_TURNS if case["graph"] else ("eager",) * EXCHANGES
        if case["graph"]:
            rc = L.gmt_rt_stream_begin_capture(rt.stream)
            if rc != 0 and not rt.hip:
                return "skipped: no stream capture on this backend"
            rt.ok(rc, "begin capture")
            rt.ok(L.gmt_ipc_exchange(ctypes.byref(plan), rt.stream), "captured gmt_ipc_exchange")
            rt.ok(L.gmt_rt_stream_end_capture(rt.stream, ctypes.byref(graph)), "end capture")
            rt.sync()
            compare(0, "after the capture (recorded, not run)")
        prev = {}
        try:
            for e, turn in enumerate(turns, start=1):
                slot = e & 1
                for i, c in enumerate(sends):  # fresh sources
                    n = extent(c)
                    model[src[i]:src[i] + n] = pattern(e, i, n)
                    rt.put(arena + src[i], model[src[i]:src[i] + n])
                for i in host_cflag:  # the host as receiver: slot e & 1 was consumed in exchange e - 2, no later
                    mflags[cflag(i)] = max(e - 2, 0)
                    rt.put(fl(cflag(i)), mflags[cflag(i):cflag(i) + 1])
                for j, c in enumerate(recvs):  # the host as sender: the slot, then "ready" (the coming epoch)
                    if c["frm"] is None:
                        a = ostage[j] + slot * ostride[j]
                        model[a:a + c["bytes"]] = pattern(e, 100 + j, c["bytes"])
                        rt.put(arena + a, model[a:a + c["bytes"]])
                        mflags[orflag(j)] = e
                        rt.put(fl(orflag(j)), mflags[orflag(j):orflag(j) + 1])
                if turn == "graph":
                    rt.ok(L.gmt_rt_graph_launch(graph, rt.stream), "graph launch")
                else:
                    rt.ok(L.gmt_ipc_exchange(ctypes.byref(plan), rt.stream), f"{name}: gmt_ipc_exchange")
                rt.sync()
                # the same exchange on the model
                msgs = {}
                for i, c in enumerate(sends):
                    msgs[i] = model[src[i] + byte_map(c)]
                    a = stage[i] + slot * stride[i]
                    model[a:a + c["bytes"]] = msgs[i]
                    if c["signal"]:
                        mflags[rflag(i)] = e
                    if e >= 2:  # the other slot still holds the previous message
                        b = stage[i] + (1 - slot) * stride[i]
                        assert np.array_equal(model[b:b + c["bytes"]], prev[i])
                for j, c in enumerate(recvs):
                    own = c["frm"] is None
                    a = (ostage[j] + slot * ostride[j]) if own else (stage[c["frm"]] + slot * stride[c["frm"]])
                    msg = model[a:a + c["bytes"]].copy()
                    model[dst[j] + byte_map(c)] = msg
                    if c["signal"]:
                        mflags[ocflag(j) if own else cflag(c["frm"])] = e
                prev = msgs
                compare(e, f"exchange {e} ({turn}, slot {slot})")
                if log is not None:
                    log.append((name, e, turn))
        finally:
            rt.L.gmt_rt_stream_synchronize(rt.stream)
            if graph.value:
                L.gmt_rt_graph_destroy(graph)
    finally:
        rt.free_all()
    return "ok"


# ------------------------------------------------------------------ refusals
def _refusals():
    ok = dict(bytes=48, src_run=0, src_ld=0, dst_run=0, dst_ld=0)
    bad = [
        ("negative bytes", dict(ok, bytes=-8)),
        ("negative src run", dict(ok, src_run=-16, src_ld=32)),
        ("negative dst run", dict(ok, dst_run=-16, dst_ld=32)),
        ("src ld < run", dict(ok, src_run=16, src_ld=8)),
        ("dst ld < run", dict(ok, dst_run=16, dst_ld=8)),
        ("src bytes % run", dict(ok, src_run=32, src_ld=64)),
        ("dst bytes % run", dict(ok, dst_run=32, dst_ld=64)),
        ("src bytes > 0xffffffff with a run", dict(ok, bytes=1 << 32, src_run=16, src_ld=16)),
        ("dst bytes > 0xffffffff with a run", dict(ok, bytes=1 << 32, dst_run=16, dst_ld=16)),
        ("both sides strided", dict(ok, src_run=16, src_ld=32, dst_run=16, dst_ld=32)),
        ("both sides strided, unequal runs", dict(ok, src_run=16, src_ld=32, dst_run=24, dst_ld=48)),
    ]
    good = [
        ("contiguous", ok),
        ("src strided", dict(ok, src_run=16, src_ld=16)),
        ("dst strided", dict(ok, dst_run=24, dst_ld=40)),
        ("4 GiB, contiguous on both sides", dict(ok, bytes=1 << 32)),
        ("zero bytes with a run", dict(ok, bytes=0, src_run=16, src_ld=32)),
    ]
    return bad, good


REFUSED, ACCEPTED = _refusals()
N_REFUSALS = 2 * len(REFUSED) + 3 + 3  # each bad channel as a send and as a receive | plan level | exchange level


def run_refusals(rt):
    """gmt_ipc_plan_init / gmt_ipc_exchange refuse these and launch nothing; returns how many were checked."""
    L = rt.L
    n = 0
    try:
        buf = rt.malloc(4096, nat.SPACE_DEVICE)
        ctl = rt.malloc(32, nat.SPACE_DEVICE)
        table = rt.malloc(int(L.gmt_ipc_table_bytes(2)), nat.SPACE_DEVICE)
        err = rt.malloc(4, nat.SPACE_PINNED)
        rt.put(ctl, np.zeros(32, np.uint8))
        rt.put(err, np.zeros(4, np.uint8))

        def chan(d):
            return nat.IpcChan(buf, buf + 2048, d["bytes"], 0, 0, None, None, d["src_run"], d["src_ld"], d["dst_run"],
                               d["dst_ld"])

        def init(ns, s, nr, r, tbl=table):
            plan = nat.IpcPlan(tbl, ctl, ctl + 8, err, 0, 0, 0, 0)
            sa = (nat.IpcChan * 1)(s) if s is not None else None
            ra = (nat.IpcChan * 1)(r) if r is not None else None
            return L.gmt_ipc_plan_init(ctypes.byref(plan), ns, sa, nr, ra), plan

        valid = chan(ACCEPTED[0][1])
        for what, d in ACCEPTED:
            assert init(1, chan(d), 0, None)[0] == 0, f"accepted as a send: {what}"
            assert init(1, valid, 1, chan(d))[0] == 0, f"accepted as a receive: {what}"
        for what, d in REFUSED:
            assert init(1, chan(d), 0, None)[0] != 0, f"not refused as a send: {what}"
            assert init(1, valid, 1, chan(d))[0] != 0, f"not refused as a receive: {what}"
            n += 2
        assert init(0, None, 0, None)[0] != 0, "n_send + n_recv == 0"
        assert init(1, valid, 0, None, tbl=None)[0] != 0, "NULL table"
        assert init(-1, valid, 2, valid)[0] != 0, "negative n_send"
        n += 3
        rc, plan = init(1, valid, 1, valid)
        assert rc == 0
        for field in ("epoch", "counters", "err"):
            p = nat.IpcPlan(plan.table, plan.epoch, plan.counters, plan.err, plan.n_send, plan.n_recv,
                            plan.send_chunks, plan.recv_chunks)
            setattr(p, field, None)
            assert L.gmt_ipc_exchange(ctypes.byref(p), rt.stream) != 0, f"gmt_ipc_exchange with a NULL {field}"
            n += 1
        rt.sync()
        state = rt.get(ctl, 8, np.uint32).tolist() + rt.get(err, 1, np.uint32).tolist()
        assert state == [0] * 9, state  # nothing ran
    finally:
        rt.free_all()
    return n


def main():
    """Every case, the refusals and the other communication kernels on the library at argv[1]; one JSON line."""
    import comm_cases

    rt = Rt(ctypes.CDLL(sys.argv[1]))
    results = {}
    try:
        for case in CASES:
            results[case["name"]] = run_case(rt, case)
        refusals = run_refusals(rt)
        comm = comm_cases.run_all(rt)
    finally:
        rt.close()
    print(json.dumps(dict(ok=True, backend=int(rt.hip), cases=len(results), refusals=refusals,
                          skipped=sorted(k for k, v in results.items() if v != "ok"), comm=comm)))


if __name__ == "__main__":
    main()
