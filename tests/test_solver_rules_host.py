"""Host side of the two solver rules that reach the kernels with ABI 7: snk_params::noncontact_order (the
limit and motor rows in the order of Bullet's quickSort on equal island ids) and snk_params::contact_erp_rule (the
contact-row ERP chosen by depth, as setupMultiBodyContactConstraint is read to choose it).  No GPU needed: the fields,
their validation in snk_create (before any HIP call), the sweep order the kernels are compiled with against the oracle's,
and the checkpoint's field-by-field parameter check."""
import json
import types

import numpy as np
import pytest


def test_fields_exist_and_default_to_zero(pkg):
    p = pkg.default_params()
    assert p.noncontact_order == 0 and p.contact_erp_rule == 0
    q = pkg.default_params(noncontact_order=1, contact_erp_rule=1)
    assert q.noncontact_order == 1 and q.contact_erp_rule == 1
    # appended at the end, behind reserved0, which keeps its name (format-2 checkpoints carry it)
    names = [n for n, _ in pkg.SnkParams._fields_]
    assert names[-3:] == ["reserved0", "noncontact_order", "contact_erp_rule"]
    import ctypes
    assert ctypes.sizeof(pkg.SnkParams) % 8 == 0
    assert p.abi_version == 7 and p.struct_size == ctypes.sizeof(pkg.SnkParams)


def test_oracle_knows_the_same_fields(pkg, oracle_mod):
    a, b = pkg.default_params(), oracle_mod.default_params()
    for name in ("noncontact_order", "contact_erp_rule"):
        assert getattr(a, name) == getattr(b, name) == 0


@pytest.mark.parametrize("over,field", [(dict(noncontact_order=2), "noncontact_order"),
                                        (dict(noncontact_order=-1), "noncontact_order"),
                                        (dict(contact_erp_rule=-1), "contact_erp_rule"),
                                        (dict(contact_erp_rule=2), "contact_erp_rule")])
def test_create_refuses_out_of_range_values(pkg, over, field):
    with pytest.raises(RuntimeError) as ei:
        pkg.Stepper(4, **over)
    assert field in str(ei.value), str(ei.value)


@pytest.mark.parametrize("over", [dict(noncontact_order=1), dict(contact_erp_rule=1),
                                  dict(noncontact_order=1, contact_order=2, contact_erp_rule=1),
                                  dict(n_modules=32, noncontact_order=1, contact_erp_rule=1)])
def test_valid_values_pass_validation(pkg, over):
    """Valid values get past the parameter checks: on a machine without a GPU the first error is the HIP device's (with
    one, the handle is created)."""
    import torch
    if torch.cuda.is_available():
        st = pkg.Stepper(4, **over)
        assert all(getattr(st.params, k) == v for k, v in over.items())
        st.close()
        return
    with pytest.raises(RuntimeError) as ei:
        pkg.Stepper(4, **over)
    msg = str(ei.value)
    assert "noncontact_order" not in msg and "contact_erp_rule" not in msg, msg
    assert "device" in msg.lower() or "hip" in msg.lower(), msg


@pytest.mark.parametrize("n", [16, 32])
def test_sweep_order_is_the_oracles(pkg, oracle_mod, n):
    """The order the kernels unroll their sweeps over (one constexpr table, read back through snk_debug_noncontact_order)
    is the oracle's quickSort on 2n equal keys: entries 0..n-1 = limit j, n..2n-1 = motor j - n."""
    from importlib import import_module
    lib = import_module("bullet-envs_amd._lib")
    got = lib.noncontact_order(n)
    want = oracle_mod.quicksort_equal_keys(2 * n)
    assert list(got) == list(want)
    # the first partition reverses the list: every motor comes first, then the limits in the same joint order
    assert np.all(got[:n] >= n) and np.array_equal(got[:n] - n, got[n:])
    assert not np.array_equal(got[:n] - n, np.arange(n))        # not the identity
    if n == 16:
        assert list(got[:n] - n) == [5, 4, 7, 6, 1, 0, 3, 2, 13, 12, 15, 14, 9, 8, 11, 10]


def test_hook_refuses_other_lengths(pkg):
    from importlib import import_module
    lib = import_module("bullet-envs_amd._lib")
    with pytest.raises(RuntimeError):
        lib.noncontact_order(8)


class _Z:
    """The part of np.load's NpzFile that checkpoint._check_params reads."""

    def __init__(self, d):
        self._d = d
        self.files = list(d)

    def __getitem__(self, k):
        return self._d[k]


def _z_without_new_fields(pkg):
    fields = pkg.checkpoint._params_fields(pkg.default_params())
    del fields["noncontact_order"], fields["contact_erp_rule"]
    assert "reserved0" in fields
    return _Z({"params_json": np.frombuffer(json.dumps(fields, sort_keys=True).encode(), dtype=np.uint8)})


def test_checkpoint_saves_the_fields_by_name(pkg):
    f = pkg.checkpoint._params_fields(pkg.default_params(noncontact_order=1, contact_erp_rule=1))
    assert f["noncontact_order"] == 1 and f["contact_erp_rule"] == 1


def test_old_checkpoint_loads_into_a_default_handle(pkg):
    z = _z_without_new_fields(pkg)
    pkg.checkpoint._check_params(z, types.SimpleNamespace(params=pkg.default_params()))


@pytest.mark.parametrize("field", ["noncontact_order", "contact_erp_rule"])
def test_old_checkpoint_is_refused_by_a_handle_with_a_rule_on(pkg, field):
    z = _z_without_new_fields(pkg)
    with pytest.raises(ValueError) as ei:
        pkg.checkpoint._check_params(z, types.SimpleNamespace(params=pkg.default_params(**{field: 1})))
    msg = str(ei.value)
    assert "`%s`" % field in msg and "absent: that build's default" in msg, msg
