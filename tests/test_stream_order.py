"""No GPU: tests/stream_order.py, the stream-order contract as a table, against include/fluca_hip.h -- every declared fl_* function has exactly one
row, every row speaks about every array the function is handed, the hot-path calls of a time step are `async`, and the rows that wait are the calls
the header lists as waiting and words as waiting."""
import re

import pytest

from tests import stream_order as so
from tests.test_capi_symbols import declared_functions

WAIT_WORDS = re.compile(r"[Ww]aits for the (?:handle's )?stream|[Bb]locking")


def problems(table, header):
    """what is wrong between a table and a header text -> list of sentences (empty: they agree)"""
    decl = so.declarations(header)
    out = []
    for name in sorted(set(decl) - set(table)):
        out.append(f"{name} is declared in fluca_hip.h and has no row in tests/stream_order.py")
    for name in sorted(set(table) - set(decl)):
        out.append(f"{name} has a row and is not declared in fluca_hip.h")
    for name in sorted(set(table) & set(decl)):
        cls, arrays = table[name]
        want = so.array_params(decl[name][0])
        if cls not in so.CLASSES:
            out.append(f"{name}: unknown class {cls!r}")
        if sorted(arrays) != sorted(want):
            out.append(f"{name}: the row speaks of {sorted(arrays)}, the declaration hands over {sorted(want)}")
        for a, what in arrays.items():
            if not (what in ("consumed", "copied") or (what.startswith("borrowed until ") and len(what) > 20)):
                out.append(f"{name}: {a} is {what!r}: not consumed, copied or 'borrowed until <when>'")
    return out


def test_the_table_names_every_declared_function_once_and_nothing_else():
    header = so.header_text()
    assert sorted(so.declarations(header)) == declared_functions(), "tests/stream_order.py and tests/test_capi_symbols.py parse the header differently"
    assert problems(so.TABLE, header) == []
    assert len(so.TABLE) >= 100


def test_a_missing_row_and_a_new_declaration_are_both_noticed():
    header = so.header_text()
    short = dict(so.TABLE)
    del short["fl_poisson_apply"]
    assert problems(short, header) == ["fl_poisson_apply is declared in fluca_hip.h and has no row in tests/stream_order.py"]
    longer = header.replace("int fl_poisson_destroy(fl_poisson *h);", "int fl_poisson_destroy(fl_poisson *h);\nint fl_poisson_new_call(fl_poisson *h, const double *x_dev);")
    assert problems(so.TABLE, longer) == ["fl_poisson_new_call is declared in fluca_hip.h and has no row in tests/stream_order.py"]
    grown = header.replace("int fl_poisson_apply(fl_poisson *h, const double *x_dev, double *y_dev);", "int fl_poisson_apply(fl_poisson *h, const double *x_dev, double *y_dev, const double *z_dev);")
    assert len(problems(so.TABLE, grown)) == 1 and "z_dev" in problems(so.TABLE, grown)[0]


def test_the_hot_path_of_a_time_step_is_async():
    for name in so.HOT_PATH:
        assert so.cls(name) == so.ASYNC, f"{name} is on the hot path of a time step: it must enqueue and return"
    assert len(set(so.HOT_PATH)) == len(so.HOT_PATH) == 35
    for name in so.ASYNC_ON_ONE_RANK_ONLY + so.NOT_RUN_PENDING:
        assert name in so.TABLE


def test_the_waiting_rows_are_the_calls_the_header_lists_and_words_as_waiting():
    header = so.header_text()
    waits = sorted(n for n in so.TABLE if so.cls(n) == so.WAITS)
    assert so.header_waiting_list(header) == waits
    decl = so.declarations(header)
    worded = [n for n in decl if WAIT_WORDS.search(decl[n][1])]
    assert len(worded) >= 12, worded
    for name in worded:             # where the comment right above a declaration says that it waits, the row says so
        assert so.cls(name) in (so.WAITS, so.SETUP), f"the header says {name} waits, its row says {so.cls(name)}"
    for name in so.TABLE:           # ... and no comment promises "enqueues and returns" of a row that waits
        if re.search(r"[Ee]nqueues? and returns?", decl[name][1]) and not WAIT_WORDS.search(decl[name][1]):
            assert so.cls(name) in (so.ASYNC, so.HOST), name


def test_the_header_states_what_the_issue_names():
    """copied / borrowed / read-before-return, for the arrays the header did not speak about"""
    decl = so.declarations()
    assert "COPIED" in decl["fl_momentum_set_state_v0"][1] and so.TABLE["fl_momentum_set_state_v0"][1]["v0_dev"] == "copied"
    assert "COPIED" in decl["fl_ibm_create"][1] and so.TABLE["fl_ibm_create"][1]["X_dev"] == so.TABLE["fl_ibm_update"][1]["X_dev"] == "copied"
    assert "read before the call returns" in decl["fl_momentum_add_buoyancy"][1] and so.TABLE["fl_momentum_add_buoyancy"][1]["accel"] == "copied"
    assert "read\n * before the call returns" in decl["fl_vec_mdot"][1] and so.TABLE["fl_vec_maxpy"][1]["alphas"] == "copied"
    assert "about is read" in decl["fl_ibm_force"][1]
    assert "BORROWED" in decl["fl_scalar_set_velocity"][1] and so.TABLE["fl_scalar_set_velocity"][1]["Vx_dev"].startswith("borrowed until")
    assert so.TABLE["fl_poisson_upload"][1]["host"].startswith("borrowed until fl_poisson_upload_fence")
    top = so.header_text().split("#ifndef FLUCA_HIP_H")[0]
    assert "ORDERED ON THE HANDLE'S STREAM LIKE A KERNEL LAUNCH" in top
    assert "fl_ibm_rigid_pose" not in top, "the not-covered list still names fl_ibm_rigid_pose"


def test_the_delay_constant_stands_beside_its_measurement():
    assert so.DELAY_MS >= 20.0
    if so.MEASURED_MS is not None:
        assert so.DELAY_MS >= 10.0 * so.MEASURED_MS and so.MEASURED_CASE
