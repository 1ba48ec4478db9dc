"""bench.py's measurements beside the headline, without a GPU: a plain run takes none of them; --full takes every one its shape
allows, less what --main-region-only / --no-side-legs / --no-cpu-baseline leave out."""
import bench

PLAIN = ["--gpus", "1", "--steps", "20", "--warmup", "5"]
ALL = ("side_regions", "stage_regions", "roofline_alone", "pnp_ceiling", "side_legs", "cpu_baseline")


def _extra(argv, rank=0, world=1):
    return bench.extra_measurements(bench.parse_args(argv), rank, world)


def test_plain_run_measures_the_headline_alone():
    assert not bench.parse_args(PLAIN).full
    for argv, world in ((PLAIN, 1), (PLAIN + ["--roofline-kernel", "conf"], 1), (PLAIN + ["--workload", "c4"], 1), (["--gpus", "2"], 2)):
        ex = _extra(argv, world=world)
        assert sorted(ex) == sorted(ALL) and not any(ex.values()), (argv, ex)


def test_full_takes_every_side_measurement():
    ex = _extra(PLAIN + ["--full"])
    assert all(ex[k] for k in ALL if k != "stage_regions") and not ex["stage_regions"]
    ex = _extra(PLAIN + ["--full", "--roofline-kernel", "conf"])          # the conf stage's per-kernel regions instead of roofline.alone
    assert ex["stage_regions"] and not ex["roofline_alone"]


def test_opt_outs_inside_full():
    ex = _extra(PLAIN + ["--full", "--main-region-only", "--no-cpu-baseline"])          # what a side leg's child runs
    assert not (ex["side_regions"] or ex["side_legs"] or ex["cpu_baseline"]) and ex["roofline_alone"] and ex["pnp_ceiling"]
    ex = _extra(PLAIN + ["--full", "--no-side-legs"])
    assert ex["side_regions"] and not ex["side_legs"] and ex["cpu_baseline"]
    ex = _extra(PLAIN + ["--full", "--batch", "4"])
    assert ex["side_regions"] and not ex["side_legs"]


def test_full_on_more_ranks_keeps_rank_zero_alone_for_the_child_processes():
    for rank in (0, 1):
        ex = _extra(["--gpus", "2", "--full"], rank=rank, world=2)
        assert ex["side_regions"] and ex["pnp_ceiling"] and not ex["side_legs"] and not ex["cpu_baseline"]
