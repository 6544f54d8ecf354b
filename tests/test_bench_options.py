"""bench.py's --full: a plain run does what its headline figure needs and nothing else; --full turns the extras on and the
--no-* options pick from them."""
import bench

EXTRAS = ("no_pmc", "no_cpu_baseline", "no_full_check", "no_secondary", "no_other_configs", "no_upload_rate")


def test_plain_run_has_every_extra_off():
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not a.full and all(getattr(a, k) for k in EXTRAS)
    # the --no-* options change nothing in a plain run
    b = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5", "--no-pmc", "--no-full-check"])
    assert vars(b) == dict(vars(a), no_pmc=True, no_full_check=True)


def test_full_run_has_every_extra_on_unless_opted_out():
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert a.full and not any(getattr(a, k) for k in EXTRAS)
    b = bench.parse_args(["--full", "--no-pmc", "--no-other-configs"])
    assert {k for k in EXTRAS if getattr(b, k)} == {"no_pmc", "no_other_configs"}
