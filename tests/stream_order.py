"""The stream-order contract of include/fluca_hip.h as a table: one row per declared function.  Importable without a GPU (tests/test_stream_order.py
holds the table to the header; tests/test_gpu_caller_arrays.py and tests/test_gpu_stream_order.py hold the library to the table).

Every call is ordered on the handle's stream like a kernel launch.  A row gives the call's class

  async   enqueues and returns: the host does not wait for the stream (after the first use on a handle, which may allocate and upload tables)
  waits   returns a host value, or is documented to wait: the stream has drained (as far as the call's own work) when it returns
  setup   create, destroy, allocation, communicator set-up, fl_poisson_tune_placement: may wait
  host    no GPU work

and, for every array (device or host) and every other pointer the function is handed, what becomes of it:

  consumed                 read / written in the call's own stream position (a device array) or before the call returns (a host array of a call
                           that waits, an output value): nothing of it is looked at later
  copied                   the handle keeps a copy, or the values travel with the launch: the caller may overwrite the array right away (a host
                           array: as soon as the call has returned; a device array: in stream order)
  borrowed until <when>    the handle keeps the POINTER: the memory must stay valid, and its contents are read when later calls run

The pending runs poison a `copied` array right after the call (T.release) and a `borrowed` one only after the last use the header allows.

Not run pending: the owner-rank marker calls fl_ibm_owned_select, fl_ibm_create_owned, fl_ibm_migrate and fl_ibm_owned_fetch.  The first three are
collective and wait by design (rows below: waits); fl_ibm_owned_fetch enqueues device-to-device copies and returns, but exists only on a set that
the waiting calls made."""
import os
import re
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ASYNC, WAITS, SETUP, HOST = "async", "waits", "setup", "host"
CLASSES = (ASYNC, WAITS, SETUP, HOST)
C, K = "consumed", "copied"


def B(until):
    return "borrowed until " + until


HANDLES = ("fl_poisson", "fl_momentum", "fl_ibm", "fl_scalar")          # a `T *h` of these is the object, not an array

TABLE = {}


def R(fn, cls_, /, **arrays):
    assert fn not in TABLE and cls_ in CLASSES, fn
    TABLE[fn] = (cls_, arrays)


# ---- life cycle, memory --------------------------------------------------------------------------------------------------------------------
R("fl_poisson_create", SETUP, grid=K, bc=K, decomp=K, out=C)
R("fl_poisson_destroy", SETUP)
R("fl_poisson_set_stream", HOST, hip_stream=B("the next fl_poisson_set_stream or fl_poisson_destroy"))
R("fl_poisson_synchronize", WAITS)
R("fl_poisson_barrier", WAITS)
R("fl_poisson_allreduce_sum", WAITS, host_vals=C)
R("fl_poisson_sizes", HOST, out=C)
R("fl_ksp_opts_default", HOST, o=C)
R("fl_version", HOST)
R("fl_abi_version", HOST)
R("fl_current_device", HOST, device=C)
R("fl_malloc", SETUP, dev_out=C)
R("fl_free", SETUP, dev=C)
R("fl_memcpy_h2d", WAITS, dev=C, host=C)
R("fl_memcpy_d2h", WAITS, host=C, dev=C)
R("fl_malloc_host", SETUP, host_out=C)
R("fl_free_host", SETUP, host=C)
R("fl_poisson_upload", ASYNC, dev=C, host=B("fl_poisson_upload_fence or fl_poisson_synchronize has returned"))
R("fl_poisson_upload_fence", WAITS)
R("fl_tuning_set", HOST, name=C)
R("fl_tuning_get", HOST, name=C, value=C)
R("fl_poisson_tune_placement", SETUP, probe_ms_out=C)
R("fl_poisson_vector_bytes", HOST, bytes_out=C)
# ---- BLAS-1 ----------------------------------------------------------------------------------------------------------------------------------
R("fl_vec_lincomb", ASYNC, x_dev=C, z_dev=C, y_dev=C)
R("fl_vec_dot", WAITS, x_dev=C, y_dev=C, result=C)
R("fl_vec_mdot", WAITS, x_dev=C, ys_dev=K, out=C)
R("fl_vec_maxpy", ASYNC, x_dev=C, alphas=K, ys_dev=K)
# ---- the Poisson operator, the projection, boundary vectors ----------------------------------------------------------------------------------
R("fl_poisson_apply", ASYNC, x_dev=C, y_dev=C)
R("fl_poisson_diagonal", ASYNC, d_dev=C)
R("fl_poisson_solve", WAITS, b_dev=C, x_dev=C, opts=C, stats=C)
R("fl_poisson_gershgorin", HOST, bound=C)
R("fl_poisson_rhs", ASYNC, Vx_dev=C, Vy_dev=C, Vz_dev=C, contrhs_dev=C, b_dev=C)
R("fl_poisson_project", ASYNC, p_dev=C, vx_dev=C, vy_dev=C, vz_dev=C, Vx_dev=C, Vy_dev=C, Vz_dev=C)
R("fl_poisson_gst_bc", ASYNC, pb_dev=C, V_dev=C)
R("fl_boundary_set_faces", ASYNC, plane_dev=C, face_dev=C)
R("fl_boundary_add_cells", ASYNC, plane_dev=C, cell_dev=C)
R("fl_boundary_add_faces", ASYNC, plane_dev=C, face_dev=C)
R("fl_pressure_update", ASYNC, dp_dev=C, p0_dev=C, phalf_dev=C, p_dev=C)
# ---- layouts -----------------------------------------------------------------------------------------------------------------------------------
R("fl_layout_from_dmstag_local", ASYNC, D=K, local_dev=C, out_dev=C)
R("fl_layout_to_dmstag_local", ASYNC, D=K, in_dev=C, local_dev=C)
R("fl_layout_from_dmstag_global", ASYNC, dof=K, global_dev=C, out_dev=C)
R("fl_layout_to_dmstag_global", ASYNC, dof=K, in_dev=C, global_dev=C)
R("fl_dmstag_global_entries", HOST, dof=C, entries=C)
# ---- communicators, decomposition --------------------------------------------------------------------------------------------------------------
R("fl_comm_unique_id", SETUP, out128=C)
R("fl_poisson_comm_init_rccl", SETUP, id128=K)
R("fl_poisson_comm_init_host", SETUP, ctx=B("fl_poisson_destroy"))
R("fl_poisson_comm_oneshot_handle", SETUP, ipc_handle64=C, address=C)
R("fl_poisson_comm_oneshot_attach", SETUP, handles=K, addresses=K)
R("fl_poisson_comm_oneshot_error", WAITS, error=C)
R("fl_poisson_comm_info", HOST, out=C)
R("fl_halo_plan", HOST, d=C, periodic=C, out=C)
R("fl_decomp_default", HOST, n=C, ranks=C, out=C)
R("fl_decomp_neighbor", HOST, d=C, periodic=C)
R("fl_decomp_neighbor_offset", HOST, d=C, periodic=C, offset=C)
# ---- the momentum block ----------------------------------------------------------------------------------------------------------------------
R("fl_momentum_create", SETUP, out=C)
R("fl_momentum_destroy", SETUP)
R("fl_momentum_set_state", ASYNC, V0_dev=K, v0interp_dev=K)
R("fl_momentum_set_state_v0", ASYNC, V0_dev=K, v0interp_dev=K, v0_dev=K)
R("fl_momentum_set_coefficients", ASYNC)
R("fl_momentum_apply", ASYNC, v_dev=C, y_dev=C)
R("fl_momentum_diagonal", ASYNC, d_dev=C)
R("fl_momentum_solve", WAITS, b_dev=C, x_dev=C, opts=C, stats=C)
R("fl_momentum_face_interp", ASYNC, v_dev=C, rhs_dev=C, V_dev=C)
R("fl_momentum_face_interp_scaled", ASYNC, v_dev=C, rhs_dev=C, V_dev=C)
R("fl_momentum_interp_faces", ASYNC, v_dev=C, vbc_dev=C, out_dev=C)
R("fl_momentum_interp_faces_ends", ASYNC, v_dev=C, vbc_dev=C, out_dev=C)
R("fl_momentum_rhs", ASYNC, v0_dev=C, p_dev=C, vbc_dev=C, momrhs_dev=C)
R("fl_momentum_add_buoyancy", ASYNC, phi_dev=C, accel=K, phi_ref=K, momrhs_dev=C)
R("fl_abf_jacobian_mult", ASYNC, v_dev=C, V_dev=C, p_dev=C, fv_dev=C, fV_dev=C, fp_dev=C)
R("fl_abf_apply", WAITS, momentum_opts=C, schur_opts=C, momrhs_dev=C, interprhs_dev=C, contrhs_dev=C, v_dev=C, V_dev=C, p_dev=C, stats=C)
R("fl_abf_set_ainv_types", HOST)
R("fl_abf_schur_apply", ASYNC, p_dev=C, y_dev=C)
R("fl_momentum_rowsum", ASYNC, out_dev=C)
R("fl_momentum_gershgorin", WAITS, radius=C)
R("fl_momentum_chebyshev_interval", WAITS, emin=C, emax=C)
# ---- immersed boundary -----------------------------------------------------------------------------------------------------------------------
R("fl_ibm_create", SETUP, X_dev=K, Y_dev=K, Z_dev=K, out=C)
R("fl_ibm_update", WAITS, X_dev=K, Y_dev=K, Z_dev=K)
R("fl_ibm_interp", ASYNC, u_dev=C, U_dev=C)
R("fl_ibm_spread", ASYNC, F_dev=C, dV_dev=C, f_dev=C)
R("fl_ibm_destroy", SETUP)
R("fl_ibm_owned_select", WAITS, X_dev=C, Y_dev=C, Z_dev=C, idx_out_dev=C, count_out=C)
R("fl_ibm_create_owned", WAITS, X_dev=K, Y_dev=K, Z_dev=K, gid_dev=K, out=C)
R("fl_ibm_owned_counts", HOST, out=C)
R("fl_ibm_migrate", WAITS, X_dev=K, Y_dev=K, Z_dev=K, attr_dev=K, L_local_new=C, moved=C)
R("fl_ibm_owned_fetch", ASYNC, X_dev=C, Y_dev=C, Z_dev=C, gid_dev=C, attr_out_dev=C)
R("fl_ibm_rigid_pose", ASYNC, X0_dev=C, Y0_dev=C, Z0_dev=C, centre0=K, centre=K, rotvec=K, velocity=K, omega=K, X_dev=C, Y_dev=C, Z_dev=C, Ut_dev=C)
R("fl_ibm_force", WAITS, F_dev=C, dV_dev=C, body_dev=C, about=C, force=C, torque=C)
# ---- passive scalar ----------------------------------------------------------------------------------------------------------------------------
R("fl_limiter_from_name", HOST, name=C, limiter=C)
R("fl_limiter_eval", HOST, psi=C)
R("fl_scalar_create", SETUP, bc=K, out=C)
R("fl_scalar_create_ranks", SETUP, bc=K, out=C)
R("fl_scalar_destroy", SETUP)
R("fl_scalar_set_boundary_value", HOST)
R("fl_scalar_set_limiter", HOST)
R("fl_scalar_set_diffusivity", HOST)
_VEL = B("the next fl_scalar_set_velocity: read by rhs / step / cfl / boundary_flux when THEY run")
R("fl_scalar_set_velocity", HOST, Vx_dev=_VEL, Vy_dev=_VEL, Vz_dev=_VEL)
R("fl_scalar_rhs", ASYNC, phi_dev=C, source_dev=C, out_dev=C)
R("fl_scalar_step", ASYNC, source_dev=C, phi_dev=C)
R("fl_scalar_cfl", WAITS, out=C)
R("fl_scalar_stats", WAITS, phi_dev=C, out=C)
R("fl_scalar_boundary_flux", WAITS, phi_dev=C, out=C)

# async only on ONE rank: on a decomposed handle a host-staged transport waits inside the exchange (fl_scalar_create_ranks: "collective")
ASYNC_ON_ONE_RANK_ONLY = ("fl_scalar_rhs", "fl_scalar_step")
# the hot-path calls of a time step: blocking there is a performance bug.  They must be `async` above.
HOT_PATH = (
    "fl_poisson_apply fl_poisson_rhs fl_poisson_project fl_poisson_gst_bc fl_poisson_diagonal fl_boundary_set_faces fl_boundary_add_cells "
    "fl_boundary_add_faces fl_pressure_update fl_vec_lincomb fl_vec_maxpy fl_momentum_set_state fl_momentum_set_state_v0 "
    "fl_momentum_set_coefficients fl_momentum_apply fl_momentum_diagonal fl_momentum_rowsum fl_momentum_face_interp "
    "fl_momentum_face_interp_scaled fl_momentum_interp_faces fl_momentum_interp_faces_ends fl_momentum_rhs fl_momentum_add_buoyancy "
    "fl_abf_jacobian_mult fl_abf_schur_apply fl_layout_from_dmstag_local fl_layout_to_dmstag_local fl_layout_from_dmstag_global "
    "fl_layout_to_dmstag_global fl_ibm_interp fl_ibm_spread fl_ibm_rigid_pose fl_scalar_rhs fl_scalar_step fl_poisson_upload").split()
NOT_RUN_PENDING = ("fl_ibm_owned_select", "fl_ibm_create_owned", "fl_ibm_migrate", "fl_ibm_owned_fetch")


def cls(name):
    return TABLE[name][0]


def all_async(names):
    """do all of these calls enqueue and return?  (`host` calls do no GPU work and so do not wait either)"""
    return all(cls(n) in (ASYNC, HOST) for n in names)


# ---- the header ----------------------------------------------------------------------------------------------------------------------------------

def header_text():
    return open(os.path.join(ROOT, "include", "fluca_hip.h")).read()


def declarations(src=None):
    """-> {function: ([(parameter, type text)], the comment right before the declaration)} as tests/test_capi_symbols.py finds the names"""
    src = header_text() if src is None else src
    out = {}
    blank = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), src, flags=re.S)        # same offsets, comments blanked
    for m in re.finditer(r"^[ \t]*(?:const\s+char\s*\*\s*|int\s+|void\s+)(fl_\w+)\s*\(([^;{]*?)\)\s*;", blank, flags=re.M | re.S):
        params = []
        for p in m.group(2).split(","):
            p = " ".join(p.split())
            if not p or p == "void":
                continue
            name = re.findall(r"(\w+)\s*((?:\[\w*\])?)$", p)[0]
            params.append((name[0], (p[:p.rfind(name[0])].strip() + " " + name[1]).strip()))
        before = src[:m.start()]
        c = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:#define[^\n]*\n\s*)*$", before, flags=re.S)
        assert m.group(1) not in out, m.group(1)
        out[m.group(1)] = (params, c.group(1) if c else "")
    return out


def array_params(params):
    """the parameters a row must speak about: every pointer or array that is not the handle itself"""
    out = []
    for name, ty in params:
        if "*" not in ty and "[" not in ty:
            continue
        base = ty.replace("const", "").replace("*", "").replace("[]", "").strip()
        if base in HANDLES and ty.count("*") == 1 and "[" not in ty:
            continue
        out.append(name)
    return out


def header_waiting_list(src=None):
    """the names in the header's paragraph 'These calls WAIT ...' (one list for `waits`)"""
    src = header_text() if src is None else src
    m = re.search(r"These calls WAIT for the handle's stream[^:]*:(.*?)\.\n", src, flags=re.S)
    assert m, "the header lost its list of waiting calls"
    return sorted(set(re.findall(r"\bfl_\w+", m.group(1))))


# ---- the delay of the pending runs ---------------------------------------------------------------------------------------------------------------
# Measured on an MI355X (tests/test_gpu_caller_arrays.py prints the host time of call(T) of every run; 381 cases, 158 tests): the longest host time of
# an `async` case in its ORDINARY run was MEASURED_MS, in MEASURED_CASE; the next were 1.03 ms (fl_abf_schur_apply DIAG on G1), 0.83 ms
# (fl_momentum_add_buoyancy on G1), 0.80 ms (fl_layout_from_dmstag_global on G1), then 0.3 ms and less.  In the pending runs, on a warm handle, no
# `async` case took more than 0.30 ms, and the queued sequences of tests/test_gpu_stream_order.py took 0.07 - 0.82 ms from the delay to their last call.
# The delay is ten times the longest ordinary time (and would not be under 20 ms): a loaded box stretches host times severalfold, and too short a
# delay fails the assertion that the delay was pending; it never passes a call that waited.
MEASURED_MS = 9.428
MEASURED_CASE = "G1 fl_poisson_apply, the first call of the process (code object load, first-use allocation)"
DELAY_MS = 95.0


class Delay:
    """DELAY_MS of plain work on a stream: torch.cuda._sleep, its cycle rate measured once per process with two events.  No host callback; finite."""
    _cycles_per_ms = None
    _lock = threading.Lock()

    @classmethod
    def calibrate(cls):
        import torch
        with cls._lock:
            cls._calibrate(torch)
        return cls._cycles_per_ms

    @classmethod
    def _calibrate(cls, torch):
        if cls._cycles_per_ms is None:
            torch.cuda._sleep(1000)                              # first launch: module load
            torch.cuda.synchronize()
            n, ms = 100_000, 0.0
            while ms < 2.0 and n < (1 << 30):                  # the counter's rate differs between devices by a factor of twenty: grow until it shows
                n *= 10
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                torch.cuda._sleep(n)
                b.record()
                b.synchronize()
                ms = a.elapsed_time(b)
            assert ms >= 2.0, (n, ms)
            cls._cycles_per_ms = n / ms
            print(f"stream_order.Delay: {n} cycles of torch.cuda._sleep took {ms:.2f} ms -> {DELAY_MS} ms = {int(cls._cycles_per_ms * DELAY_MS)} cycles")
        return cls._cycles_per_ms

    @classmethod
    def queue(cls, ms=None):
        """enqueue the delay on the CURRENT stream -> an event recorded right behind it"""
        import torch
        total = int(cls.calibrate() * (DELAY_MS if ms is None else ms))
        while total > 0:                                       # _sleep takes an int64, but keep each kernel short of a watchdog's patience
            step = min(total, 1 << 30)
            torch.cuda._sleep(step)
            total -= step
        e = torch.cuda.Event()
        e.record()
        return e
