"""The tuning / test hook contract of snpmi_set_kernel_variant / snpmi_get_kernel_variant (no GPU):
names, defaults, accepted values, and that a rejected set changes nothing."""
import pytest

from pysnptools_amd import _native as N

# name -> (default, a non-default accepted value)
WRITABLE = {
    "decode": (0, 3),
    "std": (0, 1),
    "diag": (1, 0),
    "extract": (0, 5),
    "syrk": (0, 36),
    "syrk_split": (0, 4),
    "dense_chunk": (0, 64),
    "dense_codes": (1, 0),
    "seg": (12288, 4096),
    "gather": (0, 1),
    "h2": (1, 0),
    "crt": (1, 2),
    "crt_block": (1, 0),
    "f64": (0, 1),
}
READ_ONLY = ("overlap_groups", "overlap_calls", "overlap_sig")
REJECTED = [("syrk", 4), ("syrk", 30), ("h2", 2), ("crt", 3), ("crt_block", 2), ("f64", 2)]


def set_hook(name, value):
    N.call("snpmi_set_kernel_variant", name.encode(), value)


@pytest.mark.parametrize("name", sorted(WRITABLE))
def test_default_and_round_trip(name):
    default, other = WRITABLE[name]
    assert N.kernel_variant(name) == default
    try:
        set_hook(name, other)
        assert N.kernel_variant(name) == other
    finally:
        set_hook(name, default)
    assert N.kernel_variant(name) == default


@pytest.mark.parametrize("name", READ_ONLY)
def test_read_only_hooks(name):
    before = N.kernel_variant(name)
    with pytest.raises(ValueError):
        set_hook(name, before + 1)
    assert N.kernel_variant(name) == before


@pytest.mark.parametrize("name,value", REJECTED)
def test_out_of_set_value_is_rejected_and_changes_nothing(name, value):
    before = N.kernel_variant(name)
    with pytest.raises(ValueError):
        set_hook(name, value)
    assert N.kernel_variant(name) == before


def test_every_accepted_syrk_value():
    try:
        for v in (0, 5, 20, 36, 71):
            set_hook("syrk", v)
            assert N.kernel_variant("syrk") == v
    finally:
        set_hook("syrk", 0)


@pytest.mark.parametrize("name", ["seg", "dense_chunk"])
def test_negative_clamps_to_zero(name):
    try:
        set_hook(name, -5)
        assert N.kernel_variant(name) == 0
    finally:
        set_hook(name, WRITABLE[name][0])


def test_unknown_name():
    with pytest.raises(ValueError):
        set_hook("part_order", 1)
    with pytest.raises(ValueError):
        N.kernel_variant("prefault")
