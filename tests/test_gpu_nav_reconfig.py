"""The navigation chain -- source, inflation, navigation function, local plan -- on one handle ACROSS RECONFIGURATION, held to
the host model of tests/nav_reconfig_cases.py (tests/test_nav_reconfig_host.py shows that every case discriminates).  The
rule: every call returns, byte for byte, what the package's numpy restatements give for the inputs and configurations of the
RUNS it rests on, whatever set_*, reset or other run came between, or it is refused with the message the code has, and a
refusal moves nothing.  Every comparison is bytes (nav_reconfig_cases.same); no tolerance anywhere.  One engine per test.

A. Reallocation and strides: the costmap window through 51 x 43 -> 37 x 29 -> 70 x 33 -> 51 x 43 and the occupancy window
   through 37 x 29 -> 45 x 31 -> 37 x 29 with the inflation radius 4 -> 7 -> 2 cells, the whole chain and every getter at each
   shape, and the previous shape's getters behind the source's new run; at a fixed shape max_path 64 -> 256 -> 32 with the
   local plan (5, 13, 8) -> (5, 52, 12) -> (3, 7, 4), three streams, buffers kept at their cap and read at the run's strides;
   movers with horizon 4 -> 0 -> 4 and switched off between a run and its getters.
B. A set_* between a run and what rests on it, one row per (change, place): the run's values, and `unchanged()` behind a
   refusal.  What the rows pinned when they were written (the parent returned a third thing in each):
     * set_costmap(another resolution) behind inflate_async: navfn_async turned the goals into cells with the resolution in
       force on the grids of the old one.  The inflation run now records its resolution (costmap-coarse-behind-inflate_async).
     * set_costmap(another origin) between costmap_async and inflate_async: the old grids got the new frame.  costmap_async
       now records its frame and inflate_async reads that record (costmap-moved-behind-source).
     * set_costmap(another resolution) + the matching set_inflation between costmap_async and inflate_async: the grid of
       0.05 m cells was inflated with the table built for 0.1 m.  The costmap run records its resolution (run_res) and
       pp_inflate_async holds the table to it: refused, PP_ERR_STATE (costmap-coarse-behind-source).
     * set_costmap(None) / set_occupancy(None) behind a complete chain: navfn_async raised although the inflated grids and
       their frame are recorded; it now answers from the record (test_the_source_switched_off).
C. A seeded walk: 6 seeds of 40 operations drawn uniformly from everything the chain offers on both sources, behind a
   complete chain, each answer held to the model."""
import pytest

import nav_reconfig_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture
def pair(pp, hip_lib):
    eng = R.engine(pp)
    yield R.Pair(pp, eng)
    eng.close()


def _all_ok(outs, getters=R.GETTERS):
    assert all(o[g][0] == "ok" for o in outs for g in getters)


# ---- A ----
@pytest.mark.parametrize("k", (0, 1), ids=R.SOURCES)
def test_the_window_through_its_shapes(pair, k):
    _all_ok(R.part_a_shapes(pair, k))


@pytest.mark.parametrize("k", (0, 1), ids=R.SOURCES)
def test_buffers_kept_at_their_cap_are_read_at_the_runs_strides(pair, k):
    _all_ok(R.part_a_strides(pair, k))


def test_movers_across_their_reconfiguration(pair):
    out = R.part_a_movers(pair)
    _all_ok(out[:4], R.GETTERS + ("local_movers",))


# ---- B ----
@pytest.mark.parametrize("name", R.ROW_NAMES)
def test_a_set_between_a_run_and_what_rests_on_it(pair, name):
    out = R.part_b_row(pair, name)
    refused = name == "costmap-coarse-behind-source"            # (the table's resolution is held to the run's)
    assert all((v[0] == "refused") == refused for v in out.values()), {g: v[0] for g, v in out.items()}
    assert ("inflate_async", "refused", "refused") in pair.log if refused else all(got != "refused" for _, _, got in pair.log)


@pytest.mark.parametrize("cfg, infl", ((R.OCC_COARSE, R.infl_cfg(4, 0.2)), (R.OCC_B, None)), ids=("resolution", "shape"))
def test_forgotten_maps_refuse_the_inflation_and_move_nothing(pair, cfg, infl):
    _all_ok([R.part_b_forgotten(pair, cfg, infl)])


@pytest.mark.parametrize("k", (0, 1), ids=R.SOURCES)
def test_the_source_switched_off(pair, k):
    _all_ok(R.part_b_source_off(pair, k))


# ---- C ----
@pytest.mark.parametrize("seed", R.WALK_SEEDS)
def test_a_seeded_walk(pair, seed):
    log = R.run_walk(pair, seed)
    assert len(log) == R.WALK_OPS
    for name, want, got in log:                                 # (hold has compared every answer already)
        assert got == ("ok" if want == "ok" else "refused" if want == "refused" else got), (name, want, got)
    print("walk", seed, {w: sum(1 for _, want, _ in log if want == w) for w in ("ok", "refused", "either")},
          "either refused:", sum(1 for _, want, got in log if want == "either" and got == "refused"))
