"""The runner both plugin tiers share (tests/plugin_scripts.py: run_case + assert_ran) cannot pass vacuously: a child that
exits non-zero fails whatever it printed, and so does one that never prints its marker.  The children import nothing of
the project and touch no device."""
import pytest

from . import plugin_scripts as S


def ran(script):
    return S.run_case(script, emulated=True, scale=1, timeout=60)


def test_a_printed_marker_and_exit_code_0_pass():
    S.assert_ran(ran('print("X_OK")'), "X_OK")


def test_a_non_zero_exit_fails_despite_the_marker():
    with pytest.raises(AssertionError):
        S.assert_ran(ran('print("X_OK"); raise SystemExit(3)'), "X_OK")


def test_a_missing_marker_fails_and_the_message_holds_the_childs_output():
    with pytest.raises(AssertionError):
        S.assert_ran(ran("pass"), "X_OK")
    with pytest.raises(AssertionError) as e:
        S.assert_ran(ran('import sys; print("child said this"); print("and this", file=sys.stderr); pass'), "X_OK")
    assert "child said this" in str(e.value) and "and this" in str(e.value)
