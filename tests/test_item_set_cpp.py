"""GPU: the C++ host layer's item sets (sbr::ItemSet in include/sbr.hpp, tests/cpp/item_set_tests.cpp) on a MovieLens-trained LSTM:
every family through a set of every seventh item equals the model's call with the complement excluded, and on(store) equals the
histories form for the slots that hold at most min(W, max_sequence_length) items.  The program checks itself; this runs it."""
import subprocess

import pytest

from sbr_rs_amd import build as hip_build
from test_capped_cpp import movielens_csv  # noqa: F401  (the fixture)


@pytest.mark.gpu
def test_cpp_item_set_matches_the_model_with_the_complement_excluded(movielens_csv):  # noqa: F811
    binary = hip_build.build_item_set_tests(verbose=False)
    p = subprocess.run([binary, movielens_csv, "20"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout, p.stderr)
    fields = dict(kv.split("=") for kv in p.stdout.split())
    assert int(fields["set"]) > 100 and int(fields["store_slots"]) > 0 and int(fields["short_rows"]) > 0
