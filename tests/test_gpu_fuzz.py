"""Fixed slices of the randomised parity runs (tests/fuzz_extract.py, fuzz_match.py, fuzz_ransac.py, fuzz_grid.py, fuzz_assoc.py, fuzz_pose.py)."""
import pytest

import fuzz_extract

pytestmark = pytest.mark.gpu


def test_extraction_stages_on_random_shapes(ctx, oracle):
    assert fuzz_extract.run(ctx, oracle, seed=20261004, cases=150) == 150


def test_matcher_on_random_ragged_batches(ctx, ctx_exp, oracle):
    import fuzz_match
    stats = {}
    assert fuzz_match.run(ctx, oracle, seed=20261006, cases=60, variants=False, stats=stats) == 60      # the product's one matcher
    assert fuzz_match.run(ctx_exp, oracle, seed=20261007, cases=60, variants=True, stats=stats) == 60   # its variants (experiments build)
    print("matcher fuzz: queries held to tests/ref_int.py:", stats)
    assert stats["queries"] > 5000, stats       # every query of every item, exactly (nothing is undecided in integers)


def test_ransac_kernels_on_random_and_degenerate_inputs(ctx, oracle):
    import fuzz_ransac
    import ref64
    stats = ref64.new_ransac_stats()
    assert fuzz_ransac.run(ctx, oracle, seed=20261005, cases=400, stats=stats) == 400
    print("RANSAC fuzz:", ref64.ransac_shares(stats))
    assert stats["pairs"] > stats["pairs_undecided"], stats      # most pairs' winner checks are held to tests/ref64.py as well


def test_grid_extractor_on_random_shapes_grids_and_content(ctx, oracle):
    import fuzz_grid
    import ref_orb
    stats = ref_orb.new_stats()
    assert fuzz_grid.run(ctx, oracle, seed=20261008, cases=60, ref_every=1, stats=stats) == 60   # and to tests/ref_orb.py
    assert stats["points"] > 2000 and stats["undecided_bits"] <= 0.01 * stats["bits"], stats
    assert stats["undecided_cells"] == 0 and stats["undecided_levels"] == 0, stats


def test_fuzz_assoc_slice(ctx, oracle):
    import fuzz_assoc
    stats = {}
    assert fuzz_assoc.run(ctx, oracle, seed=20261009, cases=40, stats=stats) == 40
    assert stats.get("held", 0) > stats.get("undecided", 0), stats      # most items are held to tests/ref64.py as well


def test_fuzz_pose_slice(ctx, oracle):
    import fuzz_pose
    stats = {}
    assert fuzz_pose.run(ctx, oracle, seed=20261010, cases=60, stats=stats) == 60
    assert stats["rt"] > 300 and stats["points"] > 3000 and stats["filter"] > 3000, stats   # held to tests/ref64.py as well
