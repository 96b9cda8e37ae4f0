"""GPU: what dfh_ctx_set_option accepts and what it refuses (difacto_amd/csrc/dfh_ctx.hip).

Every name of the call with the closed range it accepts: both ends are taken, one below and one above are DFH_ERR_ARG.  Then the
refusals that are not a range: a fwd_depth inside [4, 10] that is not 4, 5, 8 or 10, a rider slot of 3 (slots are 0 .. 2, + 4:
alone), an unknown name (the error names it), prep_priority once the preparation streams exist.  No kernel runs; a context
needs a device.
"""
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG = 1  # DFH_ERR_ARG (include/difacto_hip.h)

# name -> (lowest, highest) accepted value
RANGES = {
    "fwd_depth": (4, 10),
    "fwd_blocks": (0, 16384),
    "bwd_small_blocks": (1, 65536),
    "upd_kernel": (0, 1),
    "upd_hot_blocks": (1, 65536),
    "upd_mid_blocks": (1, 65536),
    "upd_few_blocks": (1, 65536),
    "upd_single_blocks": (1, 65536),
    "grow_initial_rows": (16, 1 << 28),
    "auc_in_update": (0, 1),
    "shard_mixed_update": (0, 1),
    "owner_per_key": (0, 1),
    "upd_split": (0, 1),
    "upd_interleave": (0, 64),
    "event_flags": (0, 1),
    "single_queue": (0, 1),
    "rider_slot_count": (0, 6),
    "rider_slot_scatter": (0, 6),
    "rider_slot_sort": (0, 6),
    "rider_slot_emit": (0, 6),
    "rider_start_lookup": (0, 100),
    "rider_start_forward": (0, 100),
    "rider_start_update": (0, 100),
    "rider_period_lookup": (1, 4096),
    "rider_period_forward": (1, 4096),
    "rider_period_update": (1, 4096),
    "prep_priority": (-1, 1),
}


@pytest.fixture(scope="module")
def capi():
    from difacto_amd import capi as m
    m.lib()
    return m


@pytest.fixture
def ctx(capi):
    c = capi.Context()
    yield c
    c.close()


def refused(capi, ctx, name, value):
    with pytest.raises(capi.DfhError) as e:
        ctx.set_option(name, value)
    assert e.value.code == ERR_ARG
    return str(e.value)


@pytest.mark.parametrize("name", sorted(RANGES))
def test_range_ends_accepted_and_neighbours_refused(capi, ctx, name):
    lo, hi = RANGES[name]
    ctx.set_option(name, hi)
    ctx.set_option(name, lo)
    refused(capi, ctx, name, lo - 1)
    refused(capi, ctx, name, hi + 1)
    ctx.set_option(name, hi)  # a refusal leaves the option usable


def test_fwd_depth_takes_its_four_values_only(capi, ctx):
    for v in (4, 5, 8, 10):
        ctx.set_option("fwd_depth", v)
    for v in (6, 7, 9):
        assert "fwd_depth" in refused(capi, ctx, "fwd_depth", v)


@pytest.mark.parametrize("stage", ["count", "scatter", "sort", "emit"])
def test_rider_slot_three_is_no_launch(capi, ctx, stage):
    refused(capi, ctx, "rider_slot_" + stage, 3)
    ctx.set_option("rider_slot_" + stage, 4)  # lookup, alone


def test_unknown_name_is_named(capi, ctx):
    assert "upd_no_such_option" in refused(capi, ctx, "upd_no_such_option", 1)
    assert "fwd_block" in refused(capi, ctx, "fwd_block", 1)  # a prefix of a name is no name


def test_prep_priority_after_the_streams_exist(capi, ctx):
    ctx.set_option("prep_priority", 0)
    ctx.set_pipeline(1)
    assert "prep_priority" in refused(capi, ctx, "prep_priority", 0)
    refused(capi, ctx, "prep_priority", 2)  # the range is checked first
