"""The mesh wrappers' input contract on host tensors: every row of ``mesh_wrapper_cases`` that a wrapper refuses before
it asks for device tensors, on one triangle.  The rows that need device tensors run in
``test_gpu_mesh_wrapper_contract.py``."""
import pytest

from tests import mesh_wrapper_cases as cases


@pytest.mark.parametrize("wrapper, rule", cases.tensor_rows(host_only=True))
def test_one_broken_tensor_rule_is_refused_by_type_and_message(wrapper, rule):
    change, error, regex, _ = cases.TENSOR_RULES[rule]
    v, f = change(*cases.tensors(cases.TRIANGLE_V, cases.TRIANGLE_F))
    with pytest.raises(error, match=regex):
        cases.WRAPPERS[wrapper](v, f)


@pytest.mark.parametrize("wrapper", sorted(cases.WRAPPERS))
def test_host_tensors_are_refused(wrapper):
    with pytest.raises(ValueError, match="device tensors"):
        cases.WRAPPERS[wrapper](*cases.tensors(cases.TRIANGLE_V, cases.TRIANGLE_F))


@pytest.mark.parametrize("wrapper, option, value", cases.option_rows(host=True))
def test_a_refused_option_is_named(wrapper, option, value):
    with pytest.raises(ValueError, match=option):
        cases.WRAPPERS[wrapper](*cases.tensors(cases.TRIANGLE_V, cases.TRIANGLE_F), **{option: value})


def test_the_table_covers_every_wrapper_and_rule():
    assert set(cases.HOST_REACHABLE) == set(cases.WRAPPERS)
    assert {rule for rules in cases.HOST_REACHABLE.values() for rule in rules} == set(cases.TENSOR_RULES)
    assert {w for w, *_ in cases.OPTION_RULES} <= set(cases.WRAPPERS)
