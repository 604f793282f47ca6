"""Python front end of the native Jacobi engine (``libgmt_engine.so``).

The flagship benchmark's step loop runs in C++ (``csrc/engine/jacobi.cpp``):
halo exchange over RCCL (one rank per GPU) or HIP IPC (several ranks per
GPU, or any same-node job) on a high-priority stream overlapped with the
interior sweep, both step parities captured into hipGraphs.  Python only does
the rendezvous: ``torch.distributed`` broadcasts a 128-byte id (the RCCL
unique id, or the name of the IPC transport's socket control plane), then
each ``run(k)`` is a single ctypes call that enqueues k graph replays — no
Python on the per-step critical path, which is what keeps small per-GPU
domains (strong scaling to 8 GPUs) from going launch-bound.

Transport choice (``transport="auto"``, or GMT_TRANSPORT in the environment):
RCCL when every rank has its own GPU, IPC when ranks share one (RCCL refuses
two ranks on one device; the reference's oversubscription mode,
mpi_daxpy.cc:43-54); on the CPU backend the socket emulation of RCCL, with
"ipc" selecting the memfd emulation of the IPC path.

Library selection: device ``cuda`` loads ``gpu_mpi_tests_amd/_lib`` (HIP,
gfx950); device ``cpu`` loads ``build/lib-host`` (the CPU backend, same ABI)
so the engine is testable without a GPU.  Both export SONAME ``libgmt.so``,
so one process can only hold one backend — mixing raises instead of silently
binding the wrong one.
"""
from __future__ import annotations

import ctypes
import math
import os

import numpy as np
import torch

from . import mg_tab
from .parallel import dist as gdist

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
HIP_ENGINE = os.path.join(_HERE, "_lib", "libgmt_engine.so")
HOST_ENGINE = os.path.join(_ROOT, "build", "lib-host", "libgmt_engine.so")

LOCAL, RCCL, IPC = 0, 1, 2
INITS = {"analytic": 0, "random": 1}  # JacobiConfig::init
SOURCES = {None: 0, "poly": 1, "random": 2, "host": 3}  # JacobiConfig::source ("host": an ndarray)
_KINDS = {"local": LOCAL, "rccl": RCCL, "ipc": IPC}
MAX_TSTEPS = 20  # GMT_TB_MAX_SWEEPS (csrc/include/gmt/kernels.h)
_libs: dict[str, ctypes.CDLL] = {}


class EngineOpts(ctypes.Structure):
    """gmt_engine_opts (csrc/include/gmt/engine.h)."""
    _fields_ = [(n, ctypes.c_int) for n in
                ("periodic", "overlap", "graph", "tsteps", "wg_waves", "seg_rows", "exact", "init",
                 "calibrate")] + [("seed", ctypes.c_int64), ("push", ctypes.c_int), ("shared", ctypes.c_int),
                                  ("source", ctypes.c_int), ("src_every", ctypes.c_int),
                                  ("source_amp", ctypes.c_double)]


class SolveOpts(ctypes.Structure):
    """gmt_engine_solve_opts (csrc/include/gmt/engine.h)."""
    _fields_ = [("tol", ctypes.c_double), ("rtol", ctypes.c_double), ("norm", ctypes.c_int),
                ("max_sweeps", ctypes.c_int), ("check_every", ctypes.c_int), ("lag", ctypes.c_int)]


class SolveResult(ctypes.Structure):
    """gmt_engine_solve_result (csrc/include/gmt/engine.h)."""
    _fields_ = [("converged", ctypes.c_int), ("sweeps", ctypes.c_int), ("checks", ctypes.c_int),
                ("residual_sweeps", ctypes.c_int), ("residual", ctypes.c_double),
                ("residual_max", ctypes.c_double), ("r0", ctypes.c_double), ("failed", ctypes.c_int)]


class CgOpts(ctypes.Structure):
    """gmt_engine_cg_opts (csrc/include/gmt/engine.h)."""
    _fields_ = [("tol", ctypes.c_double), ("rtol", ctypes.c_double), ("norm", ctypes.c_int),
                ("max_iters", ctypes.c_int), ("check_every", ctypes.c_int), ("lag", ctypes.c_int)]


class CgResult(ctypes.Structure):
    """gmt_engine_cg_result (csrc/include/gmt/engine.h)."""
    _fields_ = [("converged", ctypes.c_int), ("iters", ctypes.c_int), ("checks", ctypes.c_int),
                ("residual_iters", ctypes.c_int), ("residual", ctypes.c_double),
                ("residual_max", ctypes.c_double), ("r0", ctypes.c_double), ("true_residual", ctypes.c_double),
                ("true_residual_max", ctypes.c_double), ("failed", ctypes.c_int)]


class ChebyOpts(ctypes.Structure):
    """gmt_engine_cheby_opts (csrc/include/gmt/engine.h)."""
    _fields_ = [("tol", ctypes.c_double), ("rtol", ctypes.c_double), ("norm", ctypes.c_int),
                ("max_iters", ctypes.c_int), ("check_every", ctypes.c_int), ("lag", ctypes.c_int),
                ("rho", ctypes.c_double)]


class ChebyResult(ctypes.Structure):
    """gmt_engine_cheby_result (csrc/include/gmt/engine.h)."""
    _fields_ = [("converged", ctypes.c_int), ("iters", ctypes.c_int), ("checks", ctypes.c_int),
                ("residual_iters", ctypes.c_int), ("residual", ctypes.c_double),
                ("residual_max", ctypes.c_double), ("r0", ctypes.c_double), ("rho", ctypes.c_double),
                ("failed", ctypes.c_int)]


class MgOpts(ctypes.Structure):
    """gmt_engine_mg_opts (csrc/include/gmt/engine.h)."""
    _fields_ = [("tol", ctypes.c_double), ("rtol", ctypes.c_double), ("norm", ctypes.c_int),
                ("max_cycles", ctypes.c_int), ("check_every", ctypes.c_int), ("lag", ctypes.c_int),
                ("nu1", ctypes.c_int), ("nu2", ctypes.c_int), ("omega", ctypes.c_double),
                ("max_levels", ctypes.c_int), ("coarse_iters", ctypes.c_int), ("coarsen", ctypes.c_int),
                ("fuse", ctypes.c_int), ("smoother", ctypes.c_int), ("fuse_resid", ctypes.c_int),
                ("fuse_prolong", ctypes.c_int)]


class MgResult(ctypes.Structure):
    """gmt_engine_mg_result (csrc/include/gmt/engine.h)."""
    _fields_ = [("converged", ctypes.c_int), ("iters", ctypes.c_int), ("checks", ctypes.c_int),
                ("residual_iters", ctypes.c_int), ("residual", ctypes.c_double),
                ("residual_max", ctypes.c_double), ("r0", ctypes.c_double), ("failed", ctypes.c_int),
                ("levels", ctypes.c_int), ("coarse_ny", ctypes.c_int64), ("coarse_nx", ctypes.c_int64),
                ("coarse_iters", ctypes.c_int), ("coarse_rho", ctypes.c_double),
                ("fuse", ctypes.c_int), ("fuse_fine", ctypes.c_int), ("fuse_levels", ctypes.c_int),
                ("smoother", ctypes.c_int), ("fuse_resid", ctypes.c_int), ("resid_levels", ctypes.c_int),
                ("resid_mask", ctypes.c_int), ("fuse_prolong", ctypes.c_int), ("prolong_levels", ctypes.c_int),
                ("prolong_mask", ctypes.c_int)]


NORMS = {"l2": 0, "max": 1}  # SolveOpts::norm
COARSEN = {"nested": 0, "any": 1}  # MgOpts::coarsen
SMOOTHERS = {"jacobi": 0, "rb": 1}  # MgOpts::smoother
MG_OMEGA = {"jacobi": 0.8, "rb": 1.0}  # the damping when the caller gives none


def _mg_smoother(smoother, omega):
    """``(smoother, omega)`` checked, with the smoother's default damping for ``omega=None``."""
    if not isinstance(smoother, str) or smoother not in SMOOTHERS:
        raise ValueError(f"smoother must be one of {sorted(SMOOTHERS)}, got {smoother!r}")
    return smoother, MG_OMEGA[smoother] if omega is None else float(omega)
MG_MAX_FUSE = 4  # GMT_MG_MAX_FUSE: the largest MgOpts::fuse
CG_CHECK_EVERY = 10  # CgOpts::check_every == 0
MAX_LAG = 8


class EngineError(RuntimeError):
    pass


def load(device: str = "cuda") -> ctypes.CDLL:
    kind = "hip" if device.startswith("cuda") else "host"
    if kind in _libs:
        return _libs[kind]
    other = "host" if kind == "hip" else "hip"
    if other in _libs:
        raise EngineError(f"the {other} engine backend is already loaded in this process; "
                          f"run the {kind} engine in a separate process")
    path = HIP_ENGINE if kind == "hip" else HOST_ENGINE
    if not os.path.exists(path):
        raise EngineError(f"{path} is missing: build it with `make lib host` "
                          "(or __graft_entry__.build())")
    if kind == "hip":
        import torch  # noqa: F401  -- torch owns the HIP runtime first (see _native.py)
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    vp, i64, c_int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.gmt_engine_unique_id.argtypes = [vp]
    lib.gmt_engine_unique_id.restype = c_int
    lib.gmt_engine_control_id.argtypes = [vp]
    lib.gmt_engine_control_id.restype = c_int
    lib.gmt_engine_comm_create.argtypes = [c_int, c_int, c_int, vp]
    lib.gmt_engine_comm_create.restype = vp
    lib.gmt_engine_comm_allreduce_sum.argtypes = [vp, vp, i64, vp]
    lib.gmt_engine_comm_allreduce_sum.restype = c_int
    lib.gmt_engine_comm_name.argtypes = [vp]
    lib.gmt_engine_comm_name.restype = ctypes.c_char_p
    lib.gmt_engine_comm_destroy.argtypes = [vp]
    lib.gmt_engine_comm_destroy.restype = None
    lib.gmt_engine_jacobi_create.argtypes = [i64, i64, c_int, c_int, c_int, c_int, c_int, vp, vp]
    lib.gmt_engine_jacobi_create.restype = vp
    lib.gmt_engine_jacobi_destroy.argtypes = [vp]
    lib.gmt_engine_jacobi_destroy.restype = None
    for name in ("gmt_engine_jacobi_sync", "gmt_engine_jacobi_exchange"):
        getattr(lib, name).argtypes = [vp]
        getattr(lib, name).restype = c_int
    lib.gmt_engine_jacobi_run.argtypes = [vp, c_int]
    lib.gmt_engine_jacobi_run.restype = c_int
    lib.gmt_engine_jacobi_residual.argtypes = [vp]
    lib.gmt_engine_jacobi_residual.restype = ctypes.c_double
    lib.gmt_engine_jacobi_residual_norm.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
    lib.gmt_engine_jacobi_residual_norm.restype = c_int
    lib.gmt_engine_jacobi_solve.argtypes = [vp, ctypes.POINTER(SolveOpts), ctypes.POINTER(SolveResult)]
    lib.gmt_engine_jacobi_solve.restype = c_int
    lib.gmt_engine_jacobi_cg.argtypes = [vp, ctypes.POINTER(CgOpts), ctypes.POINTER(CgResult)]
    lib.gmt_engine_jacobi_cg.restype = c_int
    lib.gmt_engine_jacobi_cheby.argtypes = [vp, ctypes.POINTER(ChebyOpts), ctypes.POINTER(ChebyResult)]
    lib.gmt_engine_jacobi_cheby.restype = c_int
    lib.gmt_engine_jacobi_mg.argtypes = [vp, ctypes.POINTER(MgOpts), ctypes.POINTER(MgResult)]
    lib.gmt_engine_jacobi_mg.restype = c_int
    lib.gmt_engine_mg_levels2.argtypes = [ctypes.c_int64, ctypes.c_int64, c_int, c_int, c_int, c_int, vp, c_int]
    lib.gmt_engine_mg_levels2.restype = c_int
    lib.gmt_engine_jacobi_periodic.argtypes = [vp]
    lib.gmt_engine_jacobi_periodic.restype = c_int
    lib.gmt_engine_jacobi_info.argtypes = [vp, ctypes.POINTER(i64)]
    lib.gmt_engine_jacobi_info.restype = c_int
    lib.gmt_engine_jacobi_graphs.argtypes = [vp]
    lib.gmt_engine_jacobi_graphs.restype = c_int
    lib.gmt_engine_jacobi_tb_info.argtypes = [vp, c_int, ctypes.POINTER(i64)]
    lib.gmt_engine_jacobi_tb_info.restype = c_int
    lib.gmt_engine_jacobi_tb_shared.argtypes = [vp, c_int]
    lib.gmt_engine_jacobi_tb_shared.restype = c_int
    lib.gmt_engine_jacobi_plan.argtypes = [vp, c_int, ctypes.POINTER(c_int), c_int]
    lib.gmt_engine_jacobi_plan.restype = c_int
    lib.gmt_engine_jacobi_prepare.argtypes = [vp, c_int]
    lib.gmt_engine_jacobi_prepare.restype = c_int
    lib.gmt_engine_jacobi_copy_interior.argtypes = [vp, vp]
    lib.gmt_engine_jacobi_copy_interior.restype = c_int
    lib.gmt_engine_jacobi_set_source.argtypes = [vp, vp]
    lib.gmt_engine_jacobi_set_source.restype = c_int
    lib.gmt_engine_jacobi_source_plan.argtypes = [vp, c_int, ctypes.POINTER(c_int)]
    lib.gmt_engine_jacobi_source_plan.restype = c_int
    lib.gmt_engine_jacobi_compare.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_double)]
    lib.gmt_engine_jacobi_compare.restype = c_int
    lib.gmt_engine_jacobi_clock.argtypes = [vp, c_int, ctypes.POINTER(ctypes.c_double)]
    lib.gmt_engine_jacobi_clock.restype = c_int
    lib.gmt_engine_jacobi_stat.argtypes = [vp, c_int]
    lib.gmt_engine_jacobi_stat.restype = ctypes.c_double
    lib.gmt_engine_backend.restype = ctypes.c_char_p
    lib.gmt_engine_deriv_bench.argtypes = [i64, i64, c_int, c_int, c_int, c_int, c_int, vp, vp, c_int]
    lib.gmt_engine_deriv_bench.restype = c_int
    lib.gmt_engine_deriv_step_bench.argtypes = [i64, i64, c_int, c_int, c_int, c_int, c_int, vp, vp, c_int]
    lib.gmt_engine_deriv_step_bench.restype = c_int
    lib.gmt_engine_watchdog_kick.argtypes = [ctypes.c_char_p]
    lib.gmt_engine_watchdog_kick.restype = None
    lib.gmt_engine_watchdog_epitaph.argtypes = [ctypes.c_char_p, c_int]
    lib.gmt_engine_watchdog_epitaph.restype = None
    lib.gmt_engine_watchdog_timeout.argtypes = []
    lib.gmt_engine_watchdog_timeout.restype = ctypes.c_double
    # from libgmt (a dependency of the engine library: found through its handle)
    lib.gmt_jacobi5tb_group_cols.argtypes = [c_int, c_int]
    lib.gmt_jacobi5tb_group_cols.restype = i64
    got = lib.gmt_engine_backend().decode()
    if got != kind:
        raise EngineError(f"{path} bound to the {got} runtime, expected {kind} "
                          "(another libgmt.so is already loaded in this process)")
    _libs[kind] = lib
    return lib


def watchdog_kick(phase: str, device: str = "cpu") -> None:
    """Marks progress for the engine's hang watchdog (GMT_TIMEOUT seconds of
    no progress end the process with status 124 and a line naming the rank
    and the last phase; gmt/watchdog.hpp).  A no-op until an engine entry
    point has armed it."""
    load(device).gmt_engine_watchdog_kick(phase.encode()[:95])


def watchdog_epitaph(text: "str | None", code: int = 0, device: str = "cpu") -> None:
    """Last words for the hang watchdog: if it fires, ``text`` (a JSON object)
    is written to stdout with a "watchdog" field naming the stalled rank and
    phase, and the process exits with ``code`` instead of 124 ("" exits
    silently; None restores the default).  bench.py registers its result
    line once the headline is measured, so an extra that hangs cannot lose it."""
    load(device).gmt_engine_watchdog_epitaph(None if text is None else text.encode(), int(code))


def watchdog_timeout(device: str = "cpu") -> float:
    """The armed watchdog's timeout in seconds (0: not armed)."""
    return float(load(device).gmt_engine_watchdog_timeout())


def group_cols(sweeps: int, wg_waves: int = 0, device: str = "cpu") -> int:
    """Output columns one workgroup of the fused K-sweep kernel covers: the
    width of the W/E bands of a band-first (overlapped) pass."""
    return int(load(device).gmt_jacobi5tb_group_cols(int(sweeps), int(wg_waves)))


class _StdoutToStderr:
    """RCCL prints its init banner ("RCCL version : ...") on the process's
    C stdout; bench.py's driver contract is ONE JSON line on stdout, so
    communicator creation runs with fd 1 pointed at stderr."""

    def __enter__(self):
        import sys
        sys.stdout.flush()
        self._libc = ctypes.CDLL(None)
        self._libc.fflush(None)
        self._saved = os.dup(1)
        os.dup2(2, 1)
        return self

    def __exit__(self, *exc):
        import sys
        self._libc.fflush(None)
        sys.stdout.flush()
        os.dup2(self._saved, 1)
        os.close(self._saved)
        return False


def _broadcast_id(lib, env, kind: int) -> bytes:
    """Rank 0 creates the transport's 128-byte id, every rank gets it."""
    buf = ctypes.create_string_buffer(128)
    if env.rank == 0:
        err = (lib.gmt_engine_unique_id if kind == RCCL else lib.gmt_engine_control_id)(buf)
        if err:
            raise EngineError(f"transport id failed: {err}")
    obj = [bytes(buf.raw) if env.rank == 0 else None]
    if env.world_size > 1:
        torch.distributed.broadcast_object_list(obj, src=0, group=env.host_group)
    return obj[0]


def resolve_transport(env, transport: str = "auto") -> str:
    """auto -> rccl with one rank per GPU, ipc when ranks share a GPU; local
    for one rank.  GMT_ENGINE_TRANSPORT (rccl|ipc) overrides auto; so does
    GMT_TRANSPORT, the native apps' variable, when it names a transport the
    engine has (its other values — mpi-host, mpi-direct — are the apps' own
    and are ignored here with a warning)."""
    if transport not in ("auto", "local", "rccl", "ipc"):
        raise ValueError(f"transport must be auto, local, rccl or ipc, got {transport!r}")
    if transport == "auto":
        eng = os.environ.get("GMT_ENGINE_TRANSPORT", "").strip().lower()
        if eng:
            if eng not in ("auto", "rccl", "ipc"):
                raise ValueError(f"GMT_ENGINE_TRANSPORT must be auto, rccl or ipc, got {eng!r}")
            transport = eng
        else:
            app = os.environ.get("GMT_TRANSPORT", "").strip().lower()
            if app in ("rccl", "ipc"):
                transport = app
            elif app not in ("", "auto"):
                import warnings
                warnings.warn(f"GMT_TRANSPORT={app!r} is a native-app transport the engine does not have; "
                              "the engine picks its own (set GMT_ENGINE_TRANSPORT to choose)", stacklevel=2)
    if transport == "auto":
        if env.world_size == 1:
            return "local"
        return "ipc" if env.is_gpu and env.ranks_per_device > 1 else "rccl"
    if transport == "local" and env.world_size != 1:
        raise ValueError("transport 'local' needs world size 1")
    if transport == "rccl" and env.is_gpu and env.ranks_per_device > 1:
        raise ValueError(f"RCCL needs one rank per GPU ({env.ranks_per_device} ranks share one): use ipc")
    return transport


def transport_label(kind: str, env) -> str:
    """Name in reports: the CPU backend's emulations carry a -host suffix."""
    return kind if env.is_gpu or kind == "local" else f"{kind}-host"


def _transport_args(lib, env, transport: str):
    kind = _KINDS[resolve_transport(env, transport)]
    if kind == LOCAL:
        return kind, None
    return kind, ctypes.create_string_buffer(_broadcast_id(lib, env, kind), 128)


class Comm:
    """A bare communicator on the engine's transports (device collectives
    outside the solver: bench.py's DAXPY partial-sum all-reduce)."""

    def __init__(self, env=None, transport: str = "auto"):
        self.env = env or gdist.get()
        self.lib = load("cuda" if self.env.is_gpu else "cpu")
        self.kind = resolve_transport(self.env, transport)
        k, cid = _transport_args(self.lib, self.env, self.kind)
        with _StdoutToStderr():
            self.h = self.lib.gmt_engine_comm_create(self.env.rank, self.env.world_size, k, cid)
        if not self.h:
            raise EngineError("gmt_engine_comm_create failed")
        self.name = transport_label(self.lib.gmt_engine_comm_name(self.h).decode(), self.env)

    def allreduce_sum_(self, t: torch.Tensor) -> torch.Tensor:
        """In-place sum over ranks of a contiguous float64 tensor on this rank's device."""
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError("allreduce_sum_ needs a contiguous float64 tensor")
        if (t.device.type == "cuda") != self.env.is_gpu:
            raise ValueError(f"tensor on {t.device}, communicator on {self.env.device}")
        stream = torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else None
        err = self.lib.gmt_engine_comm_allreduce_sum(self.h, t.data_ptr(), t.numel(), stream)
        if err:
            raise EngineError(f"all-reduce failed: {err}")
        return t

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.gmt_engine_comm_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass


class NativeJacobi:
    """Distributed 2-D Jacobi (fp64) on the native engine: one rank per GPU
    (RCCL) or several ranks per GPU (IPC)."""

    def __init__(self, ny: int, nx: int, env: "gdist.DistEnv | None" = None,
                 dims: tuple[int, int] | None = None, periodic: bool = False,
                 overlap: "bool | str" = True, graph: bool = True,
                 tblock: bool | int = False, wg_waves: int = 0, seg_rows: int = 0, exact: int = -1,
                 transport: str = "auto", init: str = "analytic", seed: int = 0, calibrate: bool = False,
                 push: bool = False, shared: int = 0, source: "str | np.ndarray | None" = None,
                 source_amp: float = 1.0, src_every: int = 0):
        """source: a Poisson source term, the sweep becomes
        ``un = 0.25*((W+E)+(S+N)) + s`` (JacobiConfig::source): None (Laplace),
        "poly" (the s for which the analytic initial field x^3 + y^2 is the
        discrete fixed point), "random" (uniform in [-source_amp, source_amp),
        a hash of the global lattice point and ``seed + 1``) or an ndarray,
        this rank's ``[ny][nx]`` share of s.  With ``tblock`` the fused
        Laplace passes stay as they are: ``run`` advances in blocks of
        ``src_every`` sweeps (0 = tsteps, else a positive multiple of it), each
        the passes of ``plan(src_every)`` and one streaming add of a block
        field computed at set-up (gmt_add2d), then single source sweeps for the
        rest (:meth:`source_plan`).
        push: the fused passes exchange their halo inline (each pass stores
        its output faces straight into the neighbours' ghost cells over IPC
        mappings, then one hand-over launch; gmt/jacobi.hpp JacobiConfig::push).
        Needs the IPC transport when a neighbour is another rank; silently the
        transport's exchange when the share is too small (``push_active``).
        With ``graph`` a full pass and its hand-over replay from one hipGraph
        per parity (``graph_fused``; the hand-over's epoch lives in device
        memory, gmt_push_sync_dev); partial passes stay eager.
        shared: gmt_tb_opts.shared of every fused pass, push passes included
        (JacobiConfig::tb_shared): -1 no shared hand-off groups, 0 the kernel's
        default (a push pass then runs the per-strip kernel), 1 / 4 groups of
        four strips, 2 of two.  Each rank decides its own launch
        (``tb_launch(k)["shared_strips"]``): a share narrower than a group
        keeps the per-strip kernel."""
        if shared not in (-1, 0, 1, 2, 4) or isinstance(shared, bool):
            raise ValueError(f"shared must be -1, 0, 1, 2 or 4, got {shared!r}")
        from .parallel.decomp import choose_dims

        self.env = env or gdist.get()
        e = self.env
        self.device = "cuda" if e.is_gpu else "cpu"
        self.lib = load(self.device)
        py, px = dims if dims else choose_dims(e.world_size, ny, nx)
        if py * px != e.world_size:
            raise ValueError(f"process grid {py}x{px} != world size {e.world_size}")
        self.ny_g, self.nx_g, self.py, self.px = ny, nx, py, px
        kind = resolve_transport(e, transport)
        if e.world_size == 1 and kind in ("rccl", "ipc"):
            # a 1-rank communicator: a periodic domain exchanges its halo with
            # itself through the transport (latency measurements)
            k = _KINDS[kind]
            cid = ctypes.create_string_buffer(_broadcast_id(self.lib, e, k), 128)
            transport = k
        else:
            # GPU: RCCL over xGMI or HIP IPC.  CPU: the host backend's
            # emulations of the same semantics (RCCL over Unix sockets,
            # csrc/host/ccl_host.cpp; IPC over memfd-shared memory), so the
            # multi-rank engine path runs and is checked without GPUs.
            transport, cid = _transport_args(self.lib, e, kind)
        ks = 1 if not tblock else (2 if tblock is True else int(tblock))
        if not 1 <= ks <= MAX_TSTEPS:
            raise ValueError(f"tblock: sweeps per fused pass must be 1..{MAX_TSTEPS}, got {ks}")
        # overlap: True / False / "auto" (time both once, every rank keeps the faster)
        auto = overlap == "auto"
        if init not in INITS:
            raise ValueError(f"init must be one of {sorted(INITS)}, got {init!r}")
        if not 0 <= int(seed) < 1 << 53:
            raise ValueError("seed must be in [0, 2^53)")
        self.init, self.seed = init, int(seed)
        src_arr = None
        if isinstance(source, np.ndarray):
            src_arr, source = source, "host"
        if source not in SOURCES:
            raise ValueError(f"source must be None, 'poly', 'random' or an ndarray, got {source!r}")
        source_amp = float(source_amp)
        if not np.isfinite(source_amp) or source_amp < 0:
            raise ValueError(f"source_amp must be finite and >= 0, got {source_amp!r}")
        if isinstance(src_every, bool) or int(src_every) < 0 or (source and ks > 1 and int(src_every) % ks):
            raise ValueError(f"src_every must be 0 or a positive multiple of the {ks} sweeps per fused pass, "
                             f"got {src_every!r}")
        self.source = source
        opts = EngineOpts(periodic=int(bool(periodic)), overlap=2 if auto else int(bool(overlap)),
                          graph=int(bool(graph)), tsteps=ks, wg_waves=int(wg_waves),
                          seg_rows=int(seg_rows), exact=int(exact), init=INITS[init],
                          calibrate=int(bool(calibrate)), seed=int(seed), push=int(bool(push)),
                          shared=int(shared), source=SOURCES[source], src_every=int(src_every),
                          source_amp=source_amp)
        with _StdoutToStderr():
            self.h = self.lib.gmt_engine_jacobi_create(ny, nx, py, px, e.rank, e.world_size, transport,
                                                       cid, ctypes.byref(opts))
        if not self.h:
            raise EngineError("gmt_engine_jacobi_create failed")
        info = (ctypes.c_int64 * 16)()
        self.lib.gmt_engine_jacobi_info(self.h, info)
        (self.nx, self.ny, self.off_x, self.off_y, self.halo_bytes, self.halo_msgs,
         graph_on, overlap_on, _, _, tb, t_ov, t_ser, exact_on, band_on, push_on) = list(info)
        self.push_active = bool(push_on)
        # overlapped fused passes run band-first (boundary bands signal, the
        # output halo travels under the interior)
        self.band_first = bool(band_on)
        self.exact = bool(exact_on)
        # overlap="auto": measured seconds per fused pass {overlap, serial} (mean over ranks)
        self.tuned = {"overlap_s": t_ov / 1e9, "serial_s": t_ser / 1e9} if auto and t_ov else None
        self.tsteps = int(tb)
        self.tblock = self.tsteps > 1
        self.graph = bool(graph_on)
        # the full fused passes replay from hipGraphs (`graph` is true as soon
        # as the single sweeps do); inline-halo passes replay with their hand-over
        self.graph_fused = bool(self.lib.gmt_engine_jacobi_graphs(self.h) & 2)
        self.overlap = bool(overlap_on)
        self.transport = transport_label(kind, e)
        self.src_every = self.source_plan(0)["src_every"]
        if src_arr is not None:
            self.set_source(src_arr)

    # ------------------------------------------------------------------
    def run(self, steps: int) -> None:
        self.lib.gmt_engine_jacobi_run(self.h, int(steps))

    def step(self) -> None:
        self.run(1)

    def plan(self, steps: int) -> list[int]:
        """Sweeps per fused pass, in launch order, that ``run(steps)`` enqueues."""
        buf = (ctypes.c_int * max(1, steps))()
        n = self.lib.gmt_engine_jacobi_plan(self.h, int(steps), buf, max(1, steps))
        return list(buf[:n])

    def source_plan(self, steps: int) -> dict:
        """What ``run(steps)`` enqueues on a source engine: ``blocks`` of
        ``src_every`` sweeps (the fused passes of ``plan(src_every)``, then the
        add of the block field) and ``tail`` single source sweeps.  All zero
        without a source; ``plan`` keeps describing Laplace passes."""
        out = (ctypes.c_int * 3)()
        if self.lib.gmt_engine_jacobi_source_plan(self.h, int(steps), out):
            raise EngineError("gmt_engine_jacobi_source_plan failed")
        return {"blocks": int(out[0]), "src_every": int(out[1]), "tail": int(out[2])}

    def set_source(self, s: np.ndarray) -> None:
        """This rank's ``[ny][nx]`` share of the sweep source of an engine made
        with an ndarray ``source`` (JacobiSolver::set_source): the block field
        is recomputed and the initial field restored.  Only before the first
        sweep (or right after :meth:`prepare`).  An array of the global shape
        is cut to this rank's share.  Collective."""
        a = np.asarray(s, dtype=np.float64)
        if a.shape == (self.ny_g, self.nx_g) and a.shape != (self.ny, self.nx):
            a = a[self.off_y:self.off_y + self.ny, self.off_x:self.off_x + self.nx]
        a = np.ascontiguousarray(a)
        if a.shape != (self.ny, self.nx):
            raise ValueError(f"set_source: this rank's share is {(self.ny, self.nx)}, got {a.shape}")
        rc = self.lib.gmt_engine_jacobi_set_source(self.h, a.ctypes.data)
        if rc:
            raise EngineError({1: "set_source needs an engine made with an ndarray source",
                               2: "set_source: a sweep has already run",
                               3: "set_source: the source is too large for the scaled levels of the fused "
                                  "passes (use exact=1)"}.get(rc, f"set_source failed: {rc}"))

    def source_setup(self) -> dict:
        """The last set-up of the block field: single source sweeps run, wall-clock
        ms, device MiB of the source and block fields, max |s| over all ranks."""
        st = self.lib.gmt_engine_jacobi_stat
        return {"sweeps": int(st(self.h, 5)), "ms": float(st(self.h, 4)), "mib": float(st(self.h, 6)) / 2 ** 20,
                "max_abs": float(st(self.h, 3))}

    def prepare(self, steps: int) -> None:
        """One pass of every pass type ``run(steps)`` uses, then the initial field again."""
        self.lib.gmt_engine_jacobi_prepare(self.h, int(steps))

    def synchronize(self) -> None:
        self.lib.gmt_engine_jacobi_sync(self.h)

    @property
    def max_abs_u0(self) -> float:
        """max |u| of the initial field over all ranks (measured on the device;
        drives the scaled-level exactness guard)."""
        return float(self.lib.gmt_engine_jacobi_stat(self.h, 0))

    def pass_cost_ms(self) -> dict:
        """A full tsteps pass: measured by a calibrated prepare() (0 before) and
        the built-in table's estimate for this share."""
        return {"measured": round(float(self.lib.gmt_engine_jacobi_stat(self.h, 1)), 4),
                "table": round(float(self.lib.gmt_engine_jacobi_stat(self.h, 2)), 4)}

    def exchange(self) -> None:
        self.lib.gmt_engine_jacobi_exchange(self.h)

    def residual(self) -> float:
        return float(self.lib.gmt_engine_jacobi_residual(self.h))

    def residual_norm(self) -> tuple[float, float]:
        """(L2, max) norm of d = J(u) - u on the current field over every rank,
        from the read-only residual kernel: unlike :meth:`residual` the field
        and the sweep count are unchanged.  Collective."""
        out = (ctypes.c_double * 2)()
        if self.lib.gmt_engine_jacobi_residual_norm(self.h, out):
            raise EngineError("gmt_engine_jacobi_residual_norm failed")
        return float(out[0]), float(out[1])

    def solve(self, tol: float = 0.0, rtol: float = 0.0, norm: str = "l2", max_sweeps: int = 0,
              check_every: int = 0, lag: int = 1) -> dict:
        """Sweep until the residual meets ``r <= max(tol, rtol * r0)`` in
        ``norm`` ("l2" or "max"; r0: the residual before any sweep) or
        ``max_sweeps`` have run (JacobiSolver::solve).  The residual is checked
        every ``check_every`` sweeps (0 = tsteps) and the host decides ``lag``
        checks behind the device, so with lag >= 1 the passes keep running
        back to back.  Returns the fields of SolveResult: ``converged``,
        ``sweeps`` (advanced: ``residual_sweeps + lag * check_every`` unless
        the cap came first), ``checks``, ``residual_sweeps`` (the deciding
        check's), ``residual``, ``residual_max``, ``r0``, ``failed`` (a
        non-finite residual).  Identical on every rank.  Collective."""
        if norm not in NORMS:
            raise ValueError(f"norm must be one of {sorted(NORMS)}, got {norm!r}")
        every = int(check_every) if check_every else self.tsteps
        if isinstance(lag, bool) or not 0 <= int(lag) <= MAX_LAG:
            raise ValueError(f"lag must be 0..{MAX_LAG}, got {lag!r}")
        if every < 1:
            raise ValueError(f"check_every must be >= 1 (0 = tsteps), got {check_every!r}")
        if int(max_sweeps) < 1 or int(max_sweeps) % every:
            raise ValueError(f"max_sweeps must be a positive multiple of check_every ({every}), got {max_sweeps!r}")
        tol, rtol = float(tol), float(rtol)
        if not (np.isfinite(tol) and np.isfinite(rtol)) or tol < 0 or rtol < 0 or not (tol > 0 or rtol > 0):
            raise ValueError("tol and rtol must be finite and >= 0, and at least one positive")
        o = SolveOpts(tol=tol, rtol=rtol, norm=NORMS[norm], max_sweeps=int(max_sweeps), check_every=every,
                      lag=int(lag))
        r = SolveResult()
        if self.lib.gmt_engine_jacobi_solve(self.h, ctypes.byref(o), ctypes.byref(r)):
            raise ValueError("gmt_engine_jacobi_solve rejected its options")
        return {n: getattr(r, n) for n, _ in SolveResult._fields_}

    def cg(self, tol: float = 0.0, rtol: float = 0.0, norm: str = "l2", max_iters: int = 0,
           check_every: int = 0, lag: int = 1) -> dict:
        """Conjugate gradients on ``(I - J) u = b`` from the current field until
        the residual meets ``r <= max(tol, rtol * r0)`` in ``norm`` ("l2" or
        "max"; r0: the residual of the starting field) or ``max_iters``
        iterations have run (JacobiSolver::cg).  The residual is the same
        ``d = J(u) [+ s] - u`` as :meth:`residual_norm`'s, carried by the CG
        recurrence; it is checked every ``check_every`` iterations (0 = 10)
        and the host decides ``lag`` checks behind the device, so with
        lag >= 1 an iteration never waits for the host.  ``tol == rtol == 0``
        runs exactly ``max_iters`` iterations (``converged`` stays 0).  The
        solution replaces the current field in place; :meth:`run` afterwards
        keeps sweeping from it.  Returns the fields of CgResult:
        ``converged``, ``iters`` (``residual_iters + lag * check_every``
        unless the cap came first), ``checks``, ``residual_iters`` (the
        deciding check's), ``residual``, ``residual_max``, ``r0``,
        ``true_residual`` / ``true_residual_max`` (:meth:`residual_norm` of
        the final field), ``failed`` (a non-finite residual).  Identical on
        every rank.  Dirichlet engines only: a periodic axis raises
        ValueError.  Collective."""
        if norm not in NORMS:
            raise ValueError(f"norm must be one of {sorted(NORMS)}, got {norm!r}")
        every = int(check_every) if check_every else CG_CHECK_EVERY
        if isinstance(lag, bool) or not 0 <= int(lag) <= MAX_LAG:
            raise ValueError(f"lag must be 0..{MAX_LAG}, got {lag!r}")
        if every < 1:
            raise ValueError(f"check_every must be >= 1 (0 = {CG_CHECK_EVERY}), got {check_every!r}")
        if int(max_iters) < 1 or int(max_iters) % every:
            raise ValueError(f"max_iters must be a positive multiple of check_every ({every}), got {max_iters!r}")
        tol, rtol = float(tol), float(rtol)
        if not (np.isfinite(tol) and np.isfinite(rtol)) or tol < 0 or rtol < 0:
            raise ValueError("tol and rtol must be finite and >= 0")
        if self.lib.gmt_engine_jacobi_periodic(self.h):
            raise ValueError("cg needs Dirichlet sides: I - J is singular on a periodic axis")
        o = CgOpts(tol=tol, rtol=rtol, norm=NORMS[norm], max_iters=int(max_iters), check_every=every, lag=int(lag))
        r = CgResult()
        if self.lib.gmt_engine_jacobi_cg(self.h, ctypes.byref(o), ctypes.byref(r)):
            raise ValueError("gmt_engine_jacobi_cg rejected its options")
        return {n: getattr(r, n) for n, _ in CgResult._fields_}

    def cheby(self, tol: float = 0.0, rtol: float = 0.0, norm: str = "l2", max_iters: int = 0,
              check_every: int = 0, lag: int = 1, rho: float = 0.0) -> dict:
        """Chebyshev semi-iteration over the sweep from the current field
        (JacobiSolver::cheby): ``u_1 = G(u_0)``,
        ``u_{k+1} = u_{k-1} + w_{k+1} (G(u_k) - u_{k-1})`` with the weights of
        :func:`cheby_weights`, until the residual of :meth:`residual_norm` meets
        ``r <= max(tol, rtol * r0)`` at a check or ``max_iters`` iterations have
        run.  CG's order of convergence at the communication of single sweeps:
        one 1-wide halo exchange and one kernel per iteration, no reductions
        between checks; the field is bitwise the same on every process grid.
        Options as :meth:`cg` (``tol == rtol == 0``: exactly ``max_iters``
        iterations).  ``rho``: the spectral radius of the sweep, 0 = the closed
        form :func:`cheby_rho` of the global interior; a supplied value must be
        finite and in (0, 1) — an over-estimate converges more slowly, an
        under-estimate can stagnate.  The residual is not monotone from one
        iteration to the next: "converged" is the first *check* that meets the
        criterion.  Every call restarts the recurrence from the current field;
        :meth:`run` afterwards keeps sweeping from it.  Returns the fields of
        ChebyResult: ``converged``, ``iters``, ``checks``, ``residual_iters``,
        ``residual``, ``residual_max``, ``r0``, ``rho`` (the value used),
        ``failed``.  Identical on every rank.  Dirichlet engines only.
        Collective."""
        if norm not in NORMS:
            raise ValueError(f"norm must be one of {sorted(NORMS)}, got {norm!r}")
        every = int(check_every) if check_every else CG_CHECK_EVERY
        if isinstance(lag, bool) or not 0 <= int(lag) <= MAX_LAG:
            raise ValueError(f"lag must be 0..{MAX_LAG}, got {lag!r}")
        if every < 1:
            raise ValueError(f"check_every must be >= 1 (0 = {CG_CHECK_EVERY}), got {check_every!r}")
        if int(max_iters) < 1 or int(max_iters) % every:
            raise ValueError(f"max_iters must be a positive multiple of check_every ({every}), got {max_iters!r}")
        tol, rtol, rho = float(tol), float(rtol), float(rho)
        if not (np.isfinite(tol) and np.isfinite(rtol)) or tol < 0 or rtol < 0:
            raise ValueError("tol and rtol must be finite and >= 0")
        if rho != 0.0 and not (np.isfinite(rho) and 0.0 < rho < 1.0):
            raise ValueError(f"rho must be 0 (the closed form) or finite and in (0, 1), got {rho!r}")
        if self.lib.gmt_engine_jacobi_periodic(self.h):
            raise ValueError("cheby needs Dirichlet sides: the spectral radius is 1 on a periodic axis")
        o = ChebyOpts(tol=tol, rtol=rtol, norm=NORMS[norm], max_iters=int(max_iters), check_every=every,
                      lag=int(lag), rho=rho)
        r = ChebyResult()
        if self.lib.gmt_engine_jacobi_cheby(self.h, ctypes.byref(o), ctypes.byref(r)):
            raise ValueError("gmt_engine_jacobi_cheby rejected its options")
        return {n: getattr(r, n) for n, _ in ChebyResult._fields_}

    def mg(self, tol: float = 0.0, rtol: float = 0.0, norm: str = "l2", max_cycles: int = 0, check_every: int = 0,
           lag: int = 1, nu: tuple = (2, 2), omega: "float | None" = None, max_levels: int = 0,
           coarse_iters: int = 0, coarsen: str = "nested", fuse: int = 0, smoother: str = "jacobi",
           fuse_resid: bool = False, fuse_prolong: bool = False) -> dict:
        """Geometric multigrid V-cycles from the current field
        (JacobiSolver::mg; :func:`serial_mg` is the definition): ``nu[0]`` /
        ``nu[1]`` damped Jacobi sweeps ``u + omega*(G(u) - u)`` before / after
        the coarse-level correction, full weighting, bilinear interpolation,
        ``coarse_iters`` Chebyshev iterations from zero on the coarsest level
        (0 = :func:`mg_coarse_iters` of its spectral radius).  Levels are those
        of :func:`mg_levels` (``max_levels`` 0 = all of them, else >= 2).
        ``coarsen="nested"`` needs ``nx + 1`` and ``ny + 1`` even on every
        level; ``coarsen="any"`` takes every lattice size: an axis of ``n``
        points coarsens to :func:`mg_coarse_extent` points on the same
        interval, and a level that is not nested transfers by linear
        interpolation with the weights of :func:`mg_axis_table` and its exact
        transpose (a level with both extents odd is the nested one, bit for
        bit).  An iteration is one cycle; criterion, ``check_every`` (0 = 1), ``lag`` and
        the fixed-count mode are :meth:`cg`'s.  The solution replaces the
        current field (the parity flips with an odd ``nu[0] + nu[1]``);
        :meth:`run` afterwards keeps sweeping from it.  The field is bitwise
        the same on every process grid.  Returns the fields of MgResult:
        ``converged``, ``iters`` (cycles), ``checks``, ``residual_iters``,
        ``residual``, ``residual_max``, ``r0``, ``failed``, ``levels``,
        ``coarse_ny``, ``coarse_nx``, ``coarse_iters``, ``coarse_rho``,
        ``fuse``, ``fuse_fine``, ``fuse_levels``, and ``smoother`` and ``omega``
        as used.
        ``smoother="rb"`` smooths with red-black Gauss-Seidel
        (gmt_mg_smooth_rb) instead of damped Jacobi: a cell is red iff the sum
        of its 1-based global indices on its level is even, a sweep is the red
        half-sweep then the black one, each ``u + omega*(G(u) - u)`` on its
        colour.  ``omega=None`` is 0.8 for ``"jacobi"`` and 1.0 for ``"rb"``.
        Under ``fuse`` a run of ``n`` sweeps is ``2n`` half-sweeps, up to
        ``fuse`` of them per memory pass; ``fuse=0`` runs each half-sweep behind
        its own exchange.
        ``fuse`` (0, or 2..4) runs up to that many sweeps of a smoothing run in
        one memory pass (gmt_mg_smooth_k) behind one exchange as wide, for the
        same bits: every level has the depth :func:`mg_fuse_depths` gives it (a
        rank needs that many cells of the level on every axis it shares, and
        level 0 the engine's ghost depth: ``tsteps=1`` keeps the fine level of
        a multi-rank engine unfused while its coarse levels fuse); ``fuse_fine``
        is level 0's depth, ``fuse_levels`` the levels of depth >= 2.
        ``fuse_resid=True`` computes the residual and its restriction in one
        memory pass (gmt_mg_resid_restrict) behind one 2-wide exchange, for the
        same bits, on every level :func:`mg_resid_levels` lists; the other
        levels run the two kernels.  ``resid_levels`` lists the levels that
        ran fused.
        ``fuse_prolong=True`` interpolates inside the first pass of the
        post-smoothing run (gmt_mg_prolong_smooth instead of gmt_mg_prolong_add
        and that pass), for the same bits, on every level
        :func:`mg_prolong_levels` lists; the other levels run the two kernels.
        ``prolong_levels`` lists the levels that ran fused.
        Identical on every rank.  ValueError on bad options, a periodic axis,
        or a problem with no coarse level (``nx + 1`` or ``ny + 1`` odd, or a
        rank that would own no coarse point).  Collective."""
        if norm not in NORMS:
            raise ValueError(f"norm must be one of {sorted(NORMS)}, got {norm!r}")
        every = int(check_every) if check_every else 1
        if isinstance(lag, bool) or not 0 <= int(lag) <= MAX_LAG:
            raise ValueError(f"lag must be 0..{MAX_LAG}, got {lag!r}")
        if every < 1:
            raise ValueError(f"check_every must be >= 1 (0 = 1), got {check_every!r}")
        if int(max_cycles) < 1 or int(max_cycles) % every:
            raise ValueError(f"max_cycles must be a positive multiple of check_every ({every}), got {max_cycles!r}")
        smoother, omega = _mg_smoother(smoother, omega)
        tol, rtol = float(tol), float(rtol)
        if not (np.isfinite(tol) and np.isfinite(rtol)) or tol < 0 or rtol < 0:
            raise ValueError("tol and rtol must be finite and >= 0")
        nu1, nu2 = (int(v) for v in nu)
        if nu1 < 0 or nu2 < 0 or nu1 + nu2 == 0:
            raise ValueError(f"nu must be two counts >= 0 with a positive sum, got {nu!r}")
        if not 0.0 < omega <= 1.0:
            raise ValueError(f"omega must be in (0, 1], got {omega!r}")
        if int(max_levels) < 0 or int(max_levels) == 1 or int(coarse_iters) < 0:
            raise ValueError("max_levels must be 0 or >= 2 and coarse_iters >= 0")
        if coarsen not in COARSEN:
            raise ValueError(f"coarsen must be one of {sorted(COARSEN)}, got {coarsen!r}")
        if isinstance(fuse, bool) or int(fuse) != fuse or not (int(fuse) == 0 or 2 <= int(fuse) <= MG_MAX_FUSE):
            raise ValueError(f"fuse must be 0 or 2..{MG_MAX_FUSE}, got {fuse!r}")
        if fuse_prolong not in (False, True):
            raise ValueError(f"fuse_prolong must be False or True, got {fuse_prolong!r}")
        o = MgOpts(tol=tol, rtol=rtol, norm=NORMS[norm], max_cycles=int(max_cycles), check_every=every, lag=int(lag),
                   nu1=nu1, nu2=nu2, omega=omega, max_levels=int(max_levels), coarse_iters=int(coarse_iters),
                   coarsen=COARSEN[coarsen], fuse=int(fuse), smoother=SMOOTHERS[smoother],
                   fuse_resid=int(bool(fuse_resid)), fuse_prolong=int(fuse_prolong))
        r = MgResult()
        rc = self.lib.gmt_engine_jacobi_mg(self.h, ctypes.byref(o), ctypes.byref(r))
        if rc == 2:
            raise ValueError("mg needs Dirichlet sides: I - J is singular on a periodic axis")
        if rc in (3, 4):
            raise ValueError("mg: no coarse level: " + (
                "nx + 1 and ny + 1 must be even" if rc == 3 else
                "a rank of the process grid would own no coarse point" if coarsen == "nested" else
                "the extents are too small or a rank of the process grid would own no coarse point"))
        if rc:
            raise ValueError("gmt_engine_jacobi_mg rejected its options")
        out = {n: getattr(r, n) for n, _ in MgResult._fields_}
        out["smoother"] = smoother
        out["omega"] = omega
        out["fuse_resid"] = bool(r.fuse_resid)
        out["resid_levels"] = [l for l in range(r.levels) if r.resid_mask >> l & 1]
        del out["resid_mask"]
        out["fuse_prolong"] = bool(r.fuse_prolong)
        out["prolong_levels"] = [l for l in range(r.levels) if r.prolong_mask >> l & 1]
        del out["prolong_mask"]
        return out

    def interior(self) -> np.ndarray:
        out = np.empty((self.ny, self.nx), dtype=np.float64)
        self.lib.gmt_engine_jacobi_copy_interior(self.h, out.ctypes.data)
        return out

    def compare(self, other: "NativeJacobi") -> tuple[float, int]:
        """Bitwise comparison of this engine's current interior with another
        engine's (same global problem and process grid), on the device:
        (max |diff| over ranks, elements whose bits differ over ranks).
        Collective: every rank calls it."""
        out = (ctypes.c_double * 2)()
        if self.lib.gmt_engine_jacobi_compare(self.h, other.h, out):
            raise EngineError("gmt_engine_jacobi_compare failed")
        return float(out[0]), int(out[1])

    def tb_launch(self, k: int) -> dict:
        """The launch shape of this rank's one-rect k-sweep pass
        (gmt_jacobi5tb_plan, nothing launched): workgroups, resident slots,
        threads per workgroup, segment rows and count, VGPRs;
        ``shared_strips``: the strips per shared hand-off group (2 or 4), 0
        for a per-strip launch (gmt_jacobi5tb_shared_path — 256 threads are a
        two-strip group or two plain strips); ``shape`` names it — for
        two-stage strips 128 threads are one strip per workgroup, 256 two
        stage-major strips, 512 four (default wg_waves) —
        csrc/kernels/jacobi5tb.hpp launch_tb / sh_launch."""
        out = (ctypes.c_int64 * 6)()
        rc = self.lib.gmt_engine_jacobi_tb_info(self.h, int(k), out)
        if rc != 0:
            return {"error": int(rc)}
        keys = ("workgroups", "resident", "threads", "seg_rows", "segments", "vgprs")
        d = dict(zip(keys, (int(v) for v in out)))
        sh = d["shared_strips"] = int(self.lib.gmt_engine_jacobi_tb_shared(self.h, int(k)))
        if k > 10 and d["threads"] in (128, 256, 512):
            if sh:
                d["shape"] = (f"shared hand-off group: {'two' if sh == 2 else 'four'} strips, stage-major waves"
                              + (", inline halo exchange" if self.push_active else ""))
            else:
                d["shape"] = {128: "one two-stage strip per workgroup",
                              256: "two two-stage strips per workgroup, stage-major waves",
                              512: "four two-stage strips per workgroup, stage-major waves"}[d["threads"]]
        return d

    def clock_reset(self) -> None:
        """Zero the fused passes' shader-clock record (stream ordered)."""
        self.lib.gmt_engine_jacobi_clock(self.h, 1, None)

    def clock(self) -> dict:
        """The clock the fused passes ran at since clock_reset(): sampled
        waves' s_memtime / s_memrealtime deltas (gmt_tb_opts.clock).  MHz is
        0 on the CPU backend or without samples (GMT_CLOCK=0)."""
        out = (ctypes.c_double * 3)()
        self.lib.gmt_engine_jacobi_clock(self.h, 0, out)
        return {"sclk_mhz": round(out[0], 1), "samples": int(out[1]), "sampled_s": round(out[2], 6)}

    @property
    def points(self) -> int:
        return self.ny_g * self.nx_g

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.gmt_engine_jacobi_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass


def deriv_bench(n_local: int = 1024, n_other: int = 512 * 1024, n_iter: int = 100,
                n_warmup: int = 5, env: "gdist.DistEnv | None" = None, transport: str = "auto",
                check: bool = False) -> dict:
    """The reference's main benchmark on the native engine (one rank per GPU,
    RCCL): ``mpi_stencil2d_gt``'s test_deriv for dim 0 and dim 1 (2-deep
    ghost faces of ``n_other`` values per neighbour — 8 MiB at the reference
    default — exchanged, then the derivative kernel, ``n_iter`` times) and
    test_sum (in-place all-reduce of 1024 doubles).  Returns this rank's
    per-exchange seconds (median/mean/min/max), bytes sent per exchange,
    err_norm, and the all-reduce median seconds.  Collective: every rank calls it.
    Transport as NativeJacobi (RCCL, IPC when ranks share a GPU).  ``check``: the
    ghost rows are compared with the analytic field after every exchange
    (``bad_ghosts`` per dim; the exchanges stay timed alone)."""
    e = env or gdist.get()
    lib = load("cuda" if e.is_gpu else "cpu")
    transport, cid = _transport_args(lib, e, transport)
    out = (ctypes.c_double * 18)()
    with _StdoutToStderr():
        err = lib.gmt_engine_deriv_bench(int(n_local), int(n_other), int(n_iter), int(n_warmup), e.rank,
                                         e.world_size, transport, cid, out, int(bool(check)))
    if err:
        raise EngineError(f"gmt_engine_deriv_bench failed: {err}")
    v = list(out)
    res = {}
    for d in (0, 1):
        o = v[6 * d:6 * d + 6]
        res[f"dim{d}"] = dict(median_s=o[0], mean_s=o[1], min_s=o[2], max_s=o[3], bytes=int(o[4]),
                              err_norm=o[5], exact_norm=v[14 + d], bad_ghosts=int(v[16 + d]))
    res["allreduce_median_s"] = v[12]
    res["allreduce_max_rel_err"] = v[13]
    res["transport"] = transport_label({LOCAL: "local", RCCL: "rccl", IPC: "ipc"}[transport], e)
    return res


def deriv_step_bench(n_local: int = 1024, n_other: int = 512 * 1024, n_iter: int = 100,
                     n_warmup: int = 5, env: "gdist.DistEnv | None" = None, transport: str = "auto",
                     check: bool = False) -> dict:
    """The two derivative tests of :func:`deriv_bench` as whole steps (halo
    exchange + derivative through to completion), timed in two interleaved
    orders: serial (blocking exchange, then the full derivative) and
    overlapped (the exchange on a high-priority stream beside the interior of
    the derivative, then the ghost-dependent bands: ``gmt_stencil5_2d_interior``
    / ``gmt_stencil5_2d_edges``).  Per dim: this rank's ``serial_median_s`` and
    ``overlap_median_s``, the last (overlapped) step's ``err_norm``, and with
    ``check`` the largest err_norm of any overlapped step (``step_err_max``)
    and the ghost cells found wrong after any exchange (``bad_ghosts``); both
    -1 without.  Collective: every rank calls it."""
    e = env or gdist.get()
    lib = load("cuda" if e.is_gpu else "cpu")
    transport, cid = _transport_args(lib, e, transport)
    out = (ctypes.c_double * 12)()
    with _StdoutToStderr():
        err = lib.gmt_engine_deriv_step_bench(int(n_local), int(n_other), int(n_iter), int(n_warmup), e.rank,
                                              e.world_size, transport, cid, out, int(bool(check)))
    if err:
        raise EngineError(f"gmt_engine_deriv_step_bench failed: {err}")
    v = list(out)
    res = {}
    for d in (0, 1):
        o = v[6 * d:6 * d + 6]
        res[f"dim{d}"] = dict(serial_median_s=o[0], overlap_median_s=o[1], err_norm=o[2], step_err_max=o[3],
                              bad_ghosts=int(o[4]), exact_norm=o[5])
    res["transport"] = transport_label({LOCAL: "local", RCCL: "rccl", IPC: "ipc"}[transport], e)
    return res


def lattice_uniform(gx: np.ndarray, gy: np.ndarray, seed: int) -> np.ndarray:
    """uniform [0, 1) of integer lattice points: the same splitmix64 hash as
    gmt_fill_poly mode 5 (csrc/kernels/reduce.hip lattice_uniform), bitwise."""
    u64 = np.uint64
    gx = np.asarray(gx, dtype=np.int64) + (1 << 30)
    gy = np.asarray(gy, dtype=np.int64) + (1 << 30)
    k = (gy.astype(u64) << u64(32)) ^ gx.astype(u64)
    k = k ^ u64(seed)
    k = k + u64(0x9E3779B97F4A7C15)
    k = (k ^ (k >> u64(30))) * u64(0xBF58476D1CE4E5B9)
    k = (k ^ (k >> u64(27))) * u64(0x94D049BB133111EB)
    k = k ^ (k >> u64(31))
    return (k >> u64(11)).astype(np.float64) * 2.0 ** -53


def initial_field(ny: int, nx: int, init: str = "analytic", seed: int = 0) -> np.ndarray:
    """The engine's initial field with its ghost ring, (ny+2) x (nx+2),
    global lattice index -1..n (gmt_fill_poly mode 4 / 5)."""
    if init == "random":
        gx = np.arange(-1, nx + 1, dtype=np.int64)[None, :]
        gy = np.arange(-1, ny + 1, dtype=np.int64)[:, None]
        return lattice_uniform(np.broadcast_to(gx, (ny + 2, nx + 2)), np.broadcast_to(gy, (ny + 2, nx + 2)), seed)
    if init != "analytic":
        raise ValueError(f"init must be analytic or random, got {init!r}")
    h = 1.0 / (max(ny, nx) + 1)
    x = (np.arange(nx + 2, dtype=np.float64) - 1.0) * h
    y = (np.arange(ny + 2, dtype=np.float64) - 1.0) * h
    return (x[None, :] * x[None, :] * x[None, :]) + (y[:, None] * y[:, None])


def source_field(ny: int, nx: int, source: "str | np.ndarray | None", seed: int = 0,
                 source_amp: float = 1.0) -> np.ndarray:
    """The engine's sweep source s over the global interior, ny x nx, bitwise:
    "poly" is gmt_fill_poly mode 7, "random" mode 6 with seed ``seed + 1``."""
    if source is None:
        return np.zeros((ny, nx))
    if isinstance(source, np.ndarray):
        return np.asarray(source, dtype=np.float64)
    if source == "poly":
        h = 1.0 / (max(ny, nx) + 1)
        x = np.arange(nx, dtype=np.float64) * h
        return np.broadcast_to((-(1.5 * x + 0.5) * h * h)[None, :], (ny, nx)).copy()
    if source == "random":
        gx = np.broadcast_to(np.arange(nx, dtype=np.int64)[None, :], (ny, nx))
        gy = np.broadcast_to(np.arange(ny, dtype=np.int64)[:, None], (ny, nx))
        return float(source_amp) * (2.0 * lattice_uniform(gx, gy, seed + 1) - 1.0)
    raise ValueError(f"source must be None, 'poly', 'random' or an ndarray, got {source!r}")


def serial_jacobi(ny: int, nx: int, steps: int, periodic: bool = False, init: str = "analytic",
                  seed: int = 0, source: "str | np.ndarray | None" = None, source_amp: float = 1.0) -> np.ndarray:
    """NumPy reference of exactly the engine's problem (init, boundary, update):
    bitwise — the engine fills x^3 + y^2 on the same integer lattice with the
    same operation order (gmt_fill_poly mode 4), or the same hashed random
    field (mode 5), and sweeps in the same order.  ``source``: the single
    source sweeps ``un = 0.25*(...) + s`` (:func:`source_field`); the engine's
    fused blocks agree with them to rounding, not bitwise."""
    u = initial_field(ny, nx, init, seed)
    un = u.copy()
    s = None if source is None else source_field(ny, nx, source, seed, source_amp)
    for _ in range(steps):
        if periodic:
            u[1:-1, 0] = u[1:-1, -2]
            u[1:-1, -1] = u[1:-1, 1]
            u[0, 1:-1] = u[-2, 1:-1]
            u[-1, 1:-1] = u[1, 1:-1]
        un[1:-1, 1:-1] = 0.25 * ((u[1:-1, :-2] + u[1:-1, 2:]) + (u[:-2, 1:-1] + u[2:, 1:-1]))
        if s is not None:
            un[1:-1, 1:-1] += s
        u, un = un, u
    return u[1:-1, 1:-1].copy()


def serial_cg(ny: int, nx: int, iters: int, init: str = "analytic", seed: int = 0,
              source: "str | np.ndarray | None" = None, source_amp: float = 1.0, keep=None):
    """NumPy definition of :meth:`NativeJacobi.cg` on the whole Dirichlet
    problem: ``iters`` conjugate-gradient iterations on ``(I - J) u = b`` from
    the engine's initial field, every cell expression in the kernels' operation
    order, the dot products by ``math.fsum``.  Returns ``(field, series)``:
    the ny x nx interior after the last iteration and the list of
    ``(sqrt(rr), max |r|)`` of the recursive residual, entry k after k
    iterations (entry 0: the starting field's).  With ``keep`` (iteration
    counts), ``field`` is instead the dict ``{k: interior after k iterations}``
    of those counts: one run serves every count a test compares at."""
    u = initial_field(ny, nx, init, seed)
    s = None if source is None else source_field(ny, nx, source, seed, source_amp)
    c = u[1:-1, 1:-1]
    o = 0.25 * ((u[1:-1, :-2] + u[1:-1, 2:]) + (u[:-2, 1:-1] + u[2:, 1:-1]))
    if s is not None:
        o = o + 1.0 * s
    r = o - c
    fsum = lambda a: math.fsum(a.ravel().tolist())  # noqa: E731
    rr = fsum(r * r)
    series = [(math.sqrt(rr), float(np.abs(r).max()))]
    p = np.zeros_like(u)
    p[1:-1, 1:-1] = r
    pc = p[1:-1, 1:-1]
    kept = {0: c.copy()} if keep is not None and 0 in keep else {}
    for it in range(iters):
        q = pc - 0.25 * ((p[1:-1, :-2] + p[1:-1, 2:]) + (p[:-2, 1:-1] + p[2:, 1:-1]))
        pq = fsum(pc * q)
        alpha = rr / pq if pq > 0 else 0.0
        c += alpha * pc
        r -= alpha * q
        rr_new = fsum(r * r)
        series.append((math.sqrt(rr_new), float(np.abs(r).max())))
        beta = rr_new / rr if rr > 0 else 0.0
        pc[...] = r + beta * pc
        rr = rr_new
        if keep is not None and it + 1 in keep:
            kept[it + 1] = c.copy()
    return (c.copy() if keep is None else kept), series


def cheby_rho(ny: int, nx: int) -> float:
    """The spectral radius of the Laplace sweep on an ny x nx interior with a
    zero ring: ``0.5*(cos(pi/(nx+1)) + cos(pi/(ny+1)))``, the default ``rho`` of
    :meth:`NativeJacobi.cheby` (whose result reports the value it used: the two
    ``cos`` may differ by an ulp)."""
    return 0.5 * (math.cos(math.pi / (nx + 1)) + math.cos(math.pi / (ny + 1)))


def cheby_weights(rho: float, n: int) -> list:
    """``[w_1, ..., w_n]`` of :meth:`NativeJacobi.cheby`: ``w_1 = 1``,
    ``w_2 = 1/(1 - rho^2/2)``, ``w_{k+1} = 1/(1 - rho^2 w_k/4)``, in the
    engine's expression order (bit for bit its weights given the same rho)."""
    rho2 = rho * rho
    w = []
    for k in range(n):
        w.append(1.0 if k == 0 else 1.0 / (1.0 - 0.5 * rho2) if k == 1 else 1.0 / (1.0 - 0.25 * rho2 * w[-1]))
    return w


def serial_cheby(ny: int, nx: int, iters: int, rho: float, init: str = "analytic", seed: int = 0,
                 source: "str | np.ndarray | None" = None, source_amp: float = 1.0, restart_every=None,
                 keep=None, resid_every=None):
    """NumPy definition of :meth:`NativeJacobi.cheby` on the whole Dirichlet
    problem: ``iters`` Chebyshev iterations from the engine's initial field with
    the weights of :func:`cheby_weights` for ``rho``, every cell in the kernel's
    operation order (``o = 0.25*((w+e)+(n+s))``, ``o = o + 1.0*f``,
    ``t = o - v``, ``v + w*t``) — bitwise the engine's field.
    ``restart_every``: the recurrence restarts (``w_1 = 1``) every that many
    iterations, as a further ``cheby()`` call does.  Returns
    ``(field, series)``: the ny x nx interior after the last iteration — or,
    with ``keep`` (iteration counts), the dict ``{k: interior after k}`` — and,
    with ``resid_every``, the dict ``{k: (L2, max)}`` of the residual
    ``G(u) - u`` by ``math.fsum`` after every k that is a multiple of it
    (0 included)."""
    u = initial_field(ny, nx, init, seed)
    v = u.copy()
    s = None if source is None else source_field(ny, nx, source, seed, source_amp)
    period = int(restart_every) if restart_every else max(int(iters), 1)
    weights = cheby_weights(rho, min(period, max(int(iters), 1)))

    def sweep(a):
        o = 0.25 * ((a[1:-1, :-2] + a[1:-1, 2:]) + (a[:-2, 1:-1] + a[2:, 1:-1]))
        return o if s is None else o + 1.0 * s

    def resid(a):
        d = sweep(a) - a[1:-1, 1:-1]
        return math.sqrt(math.fsum((d * d).ravel().tolist())), float(np.abs(d).max())

    kept = {0: u[1:-1, 1:-1].copy()} if keep is not None and 0 in keep else {}
    series = {0: resid(u)} if resid_every else {}
    for it in range(iters):
        k = it % period
        if k == 0:
            v[1:-1, 1:-1] = sweep(u)
        else:
            pv = v[1:-1, 1:-1]
            t = sweep(u) - pv
            v[1:-1, 1:-1] = pv + weights[k] * t
        u, v = v, u
        if keep is not None and it + 1 in keep:
            kept[it + 1] = u[1:-1, 1:-1].copy()
        if resid_every and (it + 1) % resid_every == 0:
            series[it + 1] = resid(u)
    return (u[1:-1, 1:-1].copy() if keep is None else kept), series


def mg_coarse_iters(rho: float) -> int:
    """The default Chebyshev iteration count of :meth:`NativeJacobi.mg` on a
    coarsest level of spectral radius ``rho`` (the engine's loop, operation for
    operation): with ``sigma = (1 - sqrt(1 - rho^2))/rho`` and ``t = sigma``,
    the smallest ``k >= 1`` with ``2t/(1 + t^2) <= 0.1``, ``t`` multiplied by
    ``sigma`` each time ``k`` grows by one; 1 for ``rho = 0``."""
    if not rho > 0.0:
        return 1
    sigma = (1.0 - math.sqrt(1.0 - rho * rho)) / rho
    t, k = sigma, 1
    while not (2.0 * t / (1.0 + t * t) <= 0.1 or k >= 1 << 20):
        t = t * sigma
        k += 1
    return k


def mg_coarse_extent(n: int) -> int:
    """Coarse points of an axis of ``n`` fine ones under ``coarsen="any"``:
    ``(n-1)/2`` for odd ``n`` (the nested rule, spacing 2), ``n/2 - 1`` for
    even ``n`` (spacing ``(n+1)/(n/2)``)."""
    return mg_tab.coarse_extent(n)


def mg_axis_table(n: int, m: int):
    """The interpolation table of an axis with ``n`` fine and ``m`` coarse
    interior points on the same interval, the definition the engine, both
    kernel backends and :func:`serial_mg` share: arrays ``(q, t, r)`` whose
    entry ``i - 1`` belongs to fine point ``i`` (1-based),
    ``q, r = divmod(i*(m+1), n+1)`` in 64-bit integers and ``t = r/(n+1)`` by
    one fp64 division.  Fine ``i`` lies between coarse ``q`` and ``q + 1``
    (0 and m + 1 are the ring) with the weights ``1.0 - t`` and ``t``;
    :func:`mg_tab.axis_taps` is the transpose."""
    return mg_tab.axis_table(n, m)


def mg_levels(ny: int, nx: int, dims: tuple = (1, 1), max_levels: int = 0, coarsen: str = "nested",
              _shares: "list | None" = None) -> list:
    """The level table of :meth:`NativeJacobi.mg`: global ``(ny, nx)`` of every
    level, the fine one first.  ``coarsen="nested"``: a level has the coarser
    level ``((ny-1)/2, (nx-1)/2)`` while ``nx + 1`` and ``ny + 1`` are even,
    every rank of the ``dims = (py, px)`` grid keeps a coarse row and column (a
    rank owning fine columns ``[ox, ox+nx)`` owns coarse columns
    ``[ox/2, (ox+nx)/2)``) and ``max_levels`` (0: no limit) is not reached.
    ``coarsen="any"``: each axis goes to :func:`mg_coarse_extent` points while
    both stay >= 1; coarse point ``J`` of an axis belongs to the rank that owns
    fine cell ``J*(n+1) // (m+1)``; every rank keeps a coarse row and column;
    and on a level with an even extent every rank's tables must pass the
    checks of the transfer plan (3 or 4 taps, taps within 2 cells and
    interpolated coarse cells within 1 of the share) and a rank with a
    neighbour on an axis must have 2 cells there."""
    if coarsen not in COARSEN:
        raise ValueError(f"coarsen must be one of {sorted(COARSEN)}, got {coarsen!r}")

    def bounds(n, p):
        base, rem = divmod(n, p)
        return [i * base + min(i, rem) for i in range(p)] + [n]

    def any_axis(n, m, b, tables):
        cb = [int(v) for v in mg_tab.coarse_bound(n, m, b)]
        if any(c1 <= c0 for c0, c1 in zip(cb, cb[1:])):
            return None
        if tables:
            for k in range(len(b) - 1):
                if len(b) > 2 and b[k + 1] - b[k] < mg_tab.TAP_HALO:
                    return None
                try:
                    mg_tab.region_tables(n, m, b[k], b[k + 1] - b[k], cb[k], cb[k + 1] - cb[k])
                except ValueError:
                    return None
        return cb

    by, bx = bounds(ny, int(dims[0])), bounds(nx, int(dims[1]))
    out = [(ny, nx)]
    if _shares is not None:
        _shares.append((by, bx))
    while max_levels == 0 or len(out) < max_levels:
        if coarsen == "nested":
            if ny % 2 == 0 or nx % 2 == 0:
                break
            by, bx = [b // 2 for b in by], [b // 2 for b in bx]
            if any(b1 <= b0 for b in (by, bx) for b0, b1 in zip(b, b[1:])):
                break
            ny, nx = (ny - 1) // 2, (nx - 1) // 2
        else:
            my, mx = mg_tab.coarse_extent(ny), mg_tab.coarse_extent(nx)
            if my < 1 or mx < 1:
                break
            tables = ny % 2 == 0 or nx % 2 == 0
            cy, cx = any_axis(ny, my, by, tables), any_axis(nx, mx, bx, tables)
            if cy is None or cx is None:
                break
            (ny, by), (nx, bx) = (my, cy), (mx, cx)
        out.append((ny, nx))
        if _shares is not None:
            _shares.append((by, bx))
    return out


def mg_fuse_depths(ny: int, nx: int, dims: tuple, fuse: int, ghost: int, max_levels: int = 0,
                   coarsen: str = "nested") -> list:
    """The depth of every smoothing level of ``mg(fuse=...)`` (the coarsest
    level has none), level 0 first: the largest ``d <= fuse`` such that on each
    axis of the ``dims = (py, px)`` grid with more than one rank every rank
    owns at least ``d`` cells of the level (the shares of :func:`mg_levels`),
    and on level 0 ``d <= ghost`` (the engine's ghost depth, its ``tsteps``)
    when the grid has more than one rank.  1: the level smooths sweep by sweep.
    The Python model of gmt::mg_fuse_depths."""
    shares = []
    levels = mg_levels(ny, nx, dims, max_levels, coarsen, shares)
    out = []
    for l, (by, bx) in enumerate(shares[:len(levels) - 1]):
        d = max(int(fuse), 1)
        for b in (by, bx):
            if len(b) > 2:
                d = min(d, min(b1 - b0 for b0, b1 in zip(b, b[1:])))
        if l == 0 and int(dims[0]) * int(dims[1]) > 1:
            d = min(d, int(ghost))
        out.append(max(d, 1))
    return out


def mg_resid_levels(ny: int, nx: int, dims: tuple, ghost: int, max_levels: int = 0, coarsen: str = "nested") -> list:
    """The levels of ``mg(fuse_resid=True)`` whose residual and restriction run
    as one gmt_mg_resid_restrict: a restricting level of :func:`mg_levels`
    fuses iff both its extents are odd (its transfer is not table-driven),
    there is one rank or every rank owns at least 2 cells of the level on each
    axis of the ``dims = (py, px)`` grid with more than one rank, and, on level
    0 of several ranks, ``ghost >= 2`` (the engine's ghost depth, its
    ``tsteps``).  The Python model of gmt::mg_resid_levels."""
    shares = []
    levels = mg_levels(ny, nx, dims, max_levels, coarsen, shares)
    ranks = int(dims[0]) * int(dims[1])
    out = []
    for l, ((my, mx), (by, bx)) in enumerate(zip(levels[:-1], shares)):
        ok = my % 2 == 1 and mx % 2 == 1
        if ok and ranks > 1:
            ok = all(b1 - b0 >= 2 for b in (by, bx) if len(b) > 2 for b0, b1 in zip(b, b[1:]))
            ok = ok and (l > 0 or int(ghost) >= 2)
        if ok:
            out.append(l)
    return out


def mg_prolong_levels(ny: int, nx: int, dims: tuple, ghost: int, fuse: int = 0, nu2: int = 2,
                      smoother: str = "jacobi", max_levels: int = 0, coarsen: str = "nested") -> list:
    """The levels of ``mg(fuse_prolong=True)`` whose interpolation runs inside
    the first post-smoothing pass (gmt_mg_prolong_smooth).  With ``n2 = nu2``
    sweeps (``2 * nu2`` half-sweeps for ``smoother="rb"``) and
    ``c = min(n2, d)``, ``d`` the level's depth from :func:`mg_fuse_depths`, a
    level of :func:`mg_levels` that interpolates fuses iff ``nu2 >= 1``, both
    its extents are odd (its transfer is not table-driven), and there is one
    rank or every rank owns at least ``c // 2 + 1`` cells of the next coarser
    level on each axis of the ``dims = (py, px)`` grid with more than one rank.
    The Python model of gmt::mg_prolong_levels."""
    if smoother not in SMOOTHERS:
        raise ValueError(f"smoother must be one of {sorted(SMOOTHERS)}, got {smoother!r}")
    shares = []
    levels = mg_levels(ny, nx, dims, max_levels, coarsen, shares)
    depths = mg_fuse_depths(ny, nx, dims, fuse, ghost, max_levels, coarsen)
    ranks = int(dims[0]) * int(dims[1])
    n2 = int(nu2) * (2 if smoother == "rb" else 1)
    out = []
    for l, ((my, mx), d) in enumerate(zip(levels[:-1], depths)):
        ok = int(nu2) >= 1 and my % 2 == 1 and mx % 2 == 1
        if ok and ranks > 1:
            w = min(n2, d) // 2 + 1
            ok = all(b1 - b0 >= w for b in shares[l + 1] if len(b) > 2 for b0, b1 in zip(b, b[1:]))
        if ok:
            out.append(l)
    return out


def serial_mg(ny: int, nx: int, cycles: int, init: str = "analytic", seed: int = 0,
              source: "str | np.ndarray | None" = None, source_amp: float = 1.0, nu: tuple = (2, 2),
              omega: "float | None" = None, max_levels: int = 0, coarse_iters: int = 0,
              coarse_rho: "float | None" = None, keep=None, start: "np.ndarray | None" = None,
              coarsen: str = "nested", smoother: str = "jacobi"):
    """NumPy definition of :meth:`NativeJacobi.mg` on the whole Dirichlet
    problem: ``cycles`` V-cycles from the engine's initial field, every cell in
    the kernels' operation order (ops/reference.py ``mg_smooth``,
    ``mg_restrict``, ``mg_prolong_add``, and with ``coarsen="any"`` on a level
    with an even extent ``mg_restrict_tab``, ``mg_prolong_add_tab``; the
    coarsest level as :func:`serial_cheby` from zero) — bitwise the engine's field.
    ``smoother="rb"``: every smoothing sweep is ``mg_smooth_rb(h=2, par=0)`` over
    the whole level, whose first interior cell is red.  ``omega=None`` is 0.8
    for ``"jacobi"`` and 1.0 for ``"rb"``.
    ``coarse_rho``: the coarsest level's spectral radius (default
    :func:`cheby_rho`; the engine reports the value it used).  ``start``: an
    ny x nx interior to start from inside the initial field's ring, as a call
    on an engine that has already advanced does.  Returns
    ``(field, series)``: the ny x nx interior after the last cycle — or, with
    ``keep`` (cycle counts), the dict ``{k: interior after k cycles}`` — and the
    list of ``(L2, max)`` of the residual ``G(u) - u`` by ``math.fsum``, entry k
    after k cycles."""
    from .ops import reference as ref

    levels = mg_levels(ny, nx, (1, 1), max_levels, coarsen)
    if len(levels) < 2:
        raise ValueError("mg: no coarse level: " + ("nx + 1 and ny + 1 must be even" if coarsen == "nested" else
                                                    "the extents leave no coarse point"))
    nu1, nu2 = (int(v) for v in nu)
    smoother, omega = _mg_smoother(smoother, omega)

    def smooth(a, b, n, m, f):
        if smoother == "rb":
            ref.mg_smooth_rb(a, b, omega, 1, n, 1, m, 2, 0, 0, f, 0.25, 1.0)
        else:
            ref.mg_smooth(a, b, omega, 1, n, 1, m, f, 0.25, 1.0)

    rho = cheby_rho(*levels[-1]) if coarse_rho is None else float(coarse_rho)
    citers = int(coarse_iters) or mg_coarse_iters(rho)
    weights = cheby_weights(rho, citers)
    u0 = initial_field(ny, nx, init, seed)
    if start is not None:
        u0[1:-1, 1:-1] = start
    U = [[u0, u0.copy()]] + [[np.zeros((m + 2, n + 2)), np.zeros((m + 2, n + 2))] for m, n in levels[1:]]
    S = [None] + [np.zeros((m + 2, n + 2)) for m, n in levels[1:]]
    D = [np.zeros((m + 4, n + 4)) for m, n in levels]  # room for the 2-wide ring the general restriction allows
    if source is not None:
        S[0] = np.zeros((ny + 2, nx + 2))
        S[0][1:-1, 1:-1] = source_field(ny, nx, source, seed, source_amp)

    def sweep(a, f):
        o = 0.25 * ((a[1:-1, :-2] + a[1:-1, 2:]) + (a[:-2, 1:-1] + a[2:, 1:-1]))
        return o if f is None else o + 1.0 * f[1:-1, 1:-1]

    def cycle(lv, cur):
        """One cycle on level lv from U[lv][cur]; returns the buffer that holds the result."""
        (m, n), u, f = levels[lv], U[lv], S[lv]
        if lv == len(levels) - 1:
            for k in range(citers):
                a, b = u[cur], u[cur ^ 1]
                if k == 0:
                    b[1:-1, 1:-1] = sweep(a, f)
                else:
                    pv = b[1:-1, 1:-1]
                    t = sweep(a, f) - pv
                    b[1:-1, 1:-1] = pv + weights[k] * t
                cur ^= 1
            return cur
        for _ in range(nu1):
            smooth(u[cur], u[cur ^ 1], n, m, f)
            cur ^= 1
        a = u[cur]
        D[lv][2:-2, 2:-2] = sweep(a, f) - a[1:-1, 1:-1]
        tab = m % 2 == 0 or n % 2 == 0  # not nested: the table-driven transfers over the whole level
        (mc, nc) = levels[lv + 1]
        xaxis, yaxis = (n, nc, 0, n, 0, nc), (m, mc, 0, m, 0, mc)
        if tab:
            ref.mg_restrict_tab(D[lv], S[lv + 1], xaxis, yaxis, 2, 2, 1, 1)
        else:
            ref.mg_restrict(D[lv][1:-1, 1:-1], S[lv + 1], 0.25, 1, n, 1, m, 1, 1, 1, 1)
        U[lv + 1][0][...] = 0.0
        c = cycle(lv + 1, 0)
        if tab:
            ref.mg_prolong_add_tab(U[lv + 1][c], a, xaxis, yaxis, 1, 1, 1, 1)
        else:
            ref.mg_prolong_add(U[lv + 1][c], a, 1, n, 1, m, 1, 1, 1, 1)
        for _ in range(nu2):
            smooth(u[cur], u[cur ^ 1], n, m, f)
            cur ^= 1
        return cur

    def resid(a):
        d = sweep(a, S[0]) - a[1:-1, 1:-1]
        return math.sqrt(math.fsum((d * d).ravel().tolist())), float(np.abs(d).max())

    cur = 0
    kept = {0: U[0][0][1:-1, 1:-1].copy()} if keep is not None and 0 in keep else {}
    series = [resid(U[0][0])]
    for it in range(cycles):
        cur = cycle(0, cur)
        series.append(resid(U[0][cur]))
        if keep is not None and it + 1 in keep:
            kept[it + 1] = U[0][cur][1:-1, 1:-1].copy()
    return (U[0][cur][1:-1, 1:-1].copy() if keep is None else kept), series
