"""What mzh_probe_actions, mzh_saliency and mzh_param_grads refuse before any device or engine is needed: the cases
and the checks, once, for the three entry points -- they share one argument checker (rows_check, csrc/mzh_api_rows.hip).
tests/test_legality_cpu.py, test_saliency_cpu.py and test_pgrad_cpu.py each run them against their own entry point;
every text must carry that entry point's prefix.
"""
import ctypes

import pytest

# entry point -> (the text's prefix, the ctypes structure, its required pointers, its optional ones)
CALLS = {
    "mzh_probe_actions": ("probe_actions", "ProbeArgs", ("obs", "reward", "value"),
                          ("env_index", "state", "legal", "h0", "pi0", "value0", "h1", "pi1", "err_count")),
    "mzh_saliency": ("saliency", "SaliencyArgs", ("obs", "sal_policy", "sal_value"),
                     ("env_index", "logit_index", "picked", "disc_policy", "disc_value", "h0", "pi0", "value0", "err_count")),
    "mzh_param_grads": ("param_grads", "PgradArgs", ("obs", "action", "delta1", "delta2", "act", "h0", "z1"),
                        ("env_index", "policy_logit", "h1", "pi0", "value0", "reward", "objective", "grad", "err_count")),
}
# a buffer one call requires only beside another: state, because valid_args gives legal
ALSO_REQUIRED = {"mzh_probe_actions": ("state",), "mzh_saliency": (), "mzh_param_grads": ()}
MULTI_ERRORS = [("net_index", None, "net_index is NULL"), ("n_networks", 0, "n_networks=0"),
                ("n_networks", -1, "n_networks=-1"), ("n_networks", 257, "n_networks=257")]


def argument_errors(call):
    """(field, value, text) of every argument alone that the call refuses"""
    return [(f, None, "required buffer is NULL") for f in CALLS[call][2] + ALSO_REQUIRED[call]] + [
        ("n", 0, "bad n=0"), ("n", -2, "bad n=-2"), ("B", 0, "B=0"), ("B", -1, "B=-1"),
        ("flags", 1, "flags=0x1"), ("flags", 2, "flags=0x2"), ("flags", 64, "flags=0x40"), ("flags", 128 | 16, "flags=0x90")]


def valid_args(lib, call):
    """arguments that pass every argument check (the pointers are never dereferenced by the checks)"""
    _, struct, required, optional = CALLS[call]
    a = getattr(lib, struct)()
    a.B, a.n, a.flags = 8, 4, 0
    assert {f[0] for f in a._fields_} == {"B", "n", "flags", *required, *optional}
    for f in required + optional:
        setattr(a, f, 0x1000)
    return a


def valid_multi(lib):
    m = lib.MultiArgs()
    m.n_networks, m.net_index, m.status = 3, 0x1000, 0x1000
    return m


def _refused(lib, call, a, multi, msg):
    fn = getattr(lib.lib(), call)
    assert fn(None, None if a is None else ctypes.byref(a), multi, None) == lib.MZH_ERR_ARG == -1
    assert lib.last_error().startswith(CALLS[call][0] + ": ") and msg in lib.last_error()


def check_argument_error(lib, call, field, value, msg):
    """refused before any launch, any device use and any look at the engine, with and without multi"""
    a = valid_args(lib, call)
    setattr(a, field, value)
    for multi in (None, ctypes.byref(valid_multi(lib))):
        _refused(lib, call, a, multi, msg)


def check_rows_beyond_the_batch_null_args_optional_outputs_and_the_tile_flags(lib, call):
    _refused(lib, call, None, None, "args is NULL")
    a = valid_args(lib, call)
    a.env_index, a.n, a.B = None, 9, 8  # without env_index row j is env j: n <= B
    _refused(lib, call, a, None, "bad n=9")
    a.n = 8  # ... and n == B passes the argument checks: the next refusal is the missing engine
    _refused(lib, call, a, None, "engine NULL")
    # every optional pointer may be NULL; the probe's state is optional without legal, whatever else is given
    for drop in [CALLS[call][3]] + ([("state", "legal")] if call == "mzh_probe_actions" else []):
        a = valid_args(lib, call)
        for f in drop:
            setattr(a, f, None)
        for flags in (0, lib.MZH_FLAG_COOP_TILE16, lib.MZH_FLAG_COOP_TILE32):
            a.flags = flags
            _refused(lib, call, a, None, "engine NULL")


def check_multi_argument_error(lib, call, field, value, msg):
    """with multi: a NULL net_index and an n_networks no set can have (a set holds 1..256 networks)"""
    m = valid_multi(lib)
    setattr(m, field, value)
    _refused(lib, call, valid_args(lib, call), ctypes.byref(m), msg)
    with pytest.raises(ValueError):
        lib.check(lib.MZH_ERR_ARG, call)
