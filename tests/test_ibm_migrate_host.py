"""No GPU: what fl_ibm_migrate / fl_ibm_owned_fetch / fl_ibm_rigid_pose (include/fluca_hip.h) and NSSetImmersedBoundaryMotion (include/fluca_host.h)
answer before any device work -- the argument checks, the ABI number that announces them.  Everything behind these checks needs markers on a device:
tests/test_gpu_ibm_migrate.py, tests/test_gpu_ibm_motion.py."""
import ctypes as C


def test_the_abi_number_announces_migration():
    from fluca_amd import capi
    assert capi.lib.fl_abi_version() >= 8 and b"abi " in capi.lib.fl_version()


def test_calls_without_a_set_are_argument_errors():
    from fluca_amd import capi
    lib = capi.lib
    Lnew, moved = C.c_int64(-1), (C.c_int64 * 2)(-1, -1)
    assert lib.fl_ibm_migrate(None, None, None, None, 0, None, C.byref(Lnew), moved) == -85          # FL_ERR_ARG_NULL
    assert Lnew.value == -1 and list(moved) == [-1, -1]
    assert lib.fl_ibm_owned_fetch(None, 0, None, None, None, None, 0, None) == -85
    z = (C.c_double * 3)()
    assert lib.fl_ibm_rigid_pose(None, 0, None, None, None, z, z, z, z, z, None, None, None, None) == -85


def test_a_motion_needs_a_set_up_solver():
    from fluca_amd import hostapi as H
    c0 = (C.c_double * 3)(0.5, 0.5, 0.5)

    @H.BodyMotionFunc
    def fn(t, centre, rotvec, velocity, omega, ctx):
        return 0

    assert H.lib.NSSetImmersedBoundaryMotion(None, c0, fn, None) == H.ERR_ARG_NULL
    ns = C.c_void_p()
    assert H.lib.NSCreate(C.byref(ns)) == 0
    assert H.lib.NSSetImmersedBoundaryMotion(ns, c0, fn, None) == H.ERR_ARG_WRONGSTATE               # before NSSetUp, and no immersed boundary
    assert H.lib.NSSetImmersedBoundaryMotion(ns, c0, None, None) == H.ERR_ARG_WRONGSTATE
    H.lib.NSDestroy(C.byref(ns))
