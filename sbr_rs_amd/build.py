"""Builds libsbr_hip.so (the gfx950 engine) in-tree with hipcc.

    python -m sbr_rs_amd.build            # incremental
    python -m sbr_rs_amd.build --force

Flags that are part of the numerics contract (sbr_numerics.h): -ffp-contract=off (every fused
multiply-add is written explicitly), no -ffast-math, default (IEEE) f32 division/sqrt and
denormal handling.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libsbr_hip.so")
SOURCES = ["sbr_kernels.hip", "sbr_steps.hip", "sbr_sort.hip", "sbr_wave.hip", "sbr_report.hip", "sbr_catalogue.hip", "sbr_sessions.hip", "sbr_engine.hip"]
HEADERS = ["sbr_kernels.h", "sbr_device.h", "sbr_wave_seq.h", "sbr_numerics.h", "sbr_approx.h", "sbr_ziggurat_tables.h", "sbr_replay_plan.h", "sbr_rank_eligible.h", os.path.join("..", "..", "include", "sbr_hip.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
         "-Wall", "-Wno-unused-function", "-Wno-unused-result", "-Wno-unused-value"] + os.environ.get("SBR_EXTRA_FLAGS", "").split()


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found")


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build(force: bool = False, verbose: bool = True) -> str:
    cc = hipcc()
    hdrs = [os.path.join(CSRC, h) for h in HEADERS] + [os.path.abspath(__file__)]
    objs = []
    for src in SOURCES:
        sp = os.path.join(CSRC, src)
        obj = os.path.join(CSRC, src.replace(".hip", ".o"))
        if force or _stale(obj, [sp] + hdrs):
            cmd = [cc] + FLAGS + ["-c", sp, "-o", obj]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
        objs.append(obj)
    if force or _stale(LIB, objs):
        cmd = [cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread", "-o", LIB] + objs + ["-ldl"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return LIB


REPO = os.path.dirname(HERE)
FACADE_SRC = os.path.join(REPO, "tests", "cpp", "facade_tests.cpp")
FACADE_BIN = os.path.join(REPO, "tests", "cpp", "_build", "facade_tests")


def _build_cpp_program(src: str, binary: str, force: bool, verbose: bool) -> str:
    cxx = shutil.which("g++") or "g++"
    deps = [src, os.path.join(REPO, "include", "sbr.hpp"), os.path.join(REPO, "include", "sbr_hip.h"), LIB]
    if force or _stale(binary, deps):
        os.makedirs(os.path.dirname(binary), exist_ok=True)
        cmd = [cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(REPO, "include"), src, "-o", binary,
               "-L" + HERE, "-lsbr_hip", "-Wl,-rpath,$ORIGIN/../../../sbr_rs_amd"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return binary


def build_facade_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's test program (include/sbr.hpp over libsbr_hip.so)."""
    return _build_cpp_program(FACADE_SRC, FACADE_BIN, force, verbose)


RECOMMEND_SRC = os.path.join(REPO, "tests", "cpp", "recommend_tests.cpp")
RECOMMEND_BIN = os.path.join(REPO, "tests", "cpp", "_build", "recommend_tests")


def build_recommend_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's top-k recommendation test program."""
    return _build_cpp_program(RECOMMEND_SRC, RECOMMEND_BIN, force, verbose)


SIMILAR_SRC = os.path.join(REPO, "tests", "cpp", "similar_tests.cpp")
SIMILAR_BIN = os.path.join(REPO, "tests", "cpp", "_build", "similar_tests")


def build_similar_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's similar_items test program."""
    return _build_cpp_program(SIMILAR_SRC, SIMILAR_BIN, force, verbose)


DIVERSE_SRC = os.path.join(REPO, "tests", "cpp", "diverse_tests.cpp")
DIVERSE_BIN = os.path.join(REPO, "tests", "cpp", "_build", "diverse_tests")


def build_diverse_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's recommend_diverse test program."""
    return _build_cpp_program(DIVERSE_SRC, DIVERSE_BIN, force, verbose)


CANDIDATES_SRC = os.path.join(REPO, "tests", "cpp", "candidates_tests.cpp")
CANDIDATES_BIN = os.path.join(REPO, "tests", "cpp", "_build", "candidates_tests")


def build_candidates_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's recommend-among / score_candidates test program."""
    return _build_cpp_program(CANDIDATES_SRC, CANDIDATES_BIN, force, verbose)


SESSIONS_SRC = os.path.join(REPO, "tests", "cpp", "sessions_tests.cpp")
SESSIONS_BIN = os.path.join(REPO, "tests", "cpp", "_build", "sessions_tests")


def build_sessions_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's session-store test program."""
    return _build_cpp_program(SESSIONS_SRC, SESSIONS_BIN, force, verbose)


SESSIONS_SEEN_SRC = os.path.join(REPO, "tests", "cpp", "sessions_seen_tests.cpp")
SESSIONS_SEEN_BIN = os.path.join(REPO, "tests", "cpp", "_build", "sessions_seen_tests")


def build_sessions_seen_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's test program of the session store's seen-item memory."""
    return _build_cpp_program(SESSIONS_SEEN_SRC, SESSIONS_SEEN_BIN, force, verbose)


SESSIONS_REPLAY_SRC = os.path.join(REPO, "tests", "cpp", "sessions_replay_tests.cpp")
SESSIONS_REPLAY_BIN = os.path.join(REPO, "tests", "cpp", "_build", "sessions_replay_tests")


def build_sessions_replay_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's test program of the session store's replay."""
    return _build_cpp_program(SESSIONS_REPLAY_SRC, SESSIONS_REPLAY_BIN, force, verbose)


RANKING_SRC = os.path.join(REPO, "tests", "cpp", "ranking_tests.cpp")
RANKING_BIN = os.path.join(REPO, "tests", "cpp", "_build", "ranking_tests")


def build_ranking_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's rank_targets / ranking_metrics test program."""
    return _build_cpp_program(RANKING_SRC, RANKING_BIN, force, verbose)


FILTERED_SRC = os.path.join(REPO, "tests", "cpp", "filtered_tests.cpp")
FILTERED_BIN = os.path.join(REPO, "tests", "cpp", "_build", "filtered_tests")


def build_filtered_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's tag-filter test program."""
    return _build_cpp_program(FILTERED_SRC, FILTERED_BIN, force, verbose)


AUDIENCE_SRC = os.path.join(REPO, "tests", "cpp", "audience_tests.cpp")
AUDIENCE_BIN = os.path.join(REPO, "tests", "cpp", "_build", "audience_tests")


def build_audience_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's audience (reverse scan) test program."""
    return _build_cpp_program(AUDIENCE_SRC, AUDIENCE_BIN, force, verbose)


SAMPLED_SRC = os.path.join(REPO, "tests", "cpp", "sampled_tests.cpp")
SAMPLED_BIN = os.path.join(REPO, "tests", "cpp", "_build", "sampled_tests")


def build_sampled_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's recommend_sampled test program."""
    return _build_cpp_program(SAMPLED_SRC, SAMPLED_BIN, force, verbose)


PARTITION_SRC = os.path.join(REPO, "tests", "cpp", "partition_tests.cpp")
PARTITION_BIN = os.path.join(REPO, "tests", "cpp", "_build", "partition_tests")


def build_partition_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's log_partition test program."""
    return _build_cpp_program(PARTITION_SRC, PARTITION_BIN, force, verbose)


ABOVE_SRC = os.path.join(REPO, "tests", "cpp", "above_tests.cpp")
ABOVE_BIN = os.path.join(REPO, "tests", "cpp", "_build", "above_tests")


def build_above_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's recommend_above / audience_above test program."""
    return _build_cpp_program(ABOVE_SRC, ABOVE_BIN, force, verbose)


TOP_SRC = os.path.join(REPO, "tests", "cpp", "top_tests.cpp")
TOP_BIN = os.path.join(REPO, "tests", "cpp", "_build", "top_tests")


def build_top_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's recommend_top / audience_top test program."""
    return _build_cpp_program(TOP_SRC, TOP_BIN, force, verbose)


CAPPED_SRC = os.path.join(REPO, "tests", "cpp", "capped_tests.cpp")
CAPPED_BIN = os.path.join(REPO, "tests", "cpp", "_build", "capped_tests")


def build_capped_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's recommend_capped test program."""
    return _build_cpp_program(CAPPED_SRC, CAPPED_BIN, force, verbose)


SEQUENCE_RANKS_SRC = os.path.join(REPO, "tests", "cpp", "sequence_ranks_tests.cpp")
SEQUENCE_RANKS_BIN = os.path.join(REPO, "tests", "cpp", "_build", "sequence_ranks_tests")


def build_sequence_ranks_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's sequence_ranks / sequence_metrics test program."""
    return _build_cpp_program(SEQUENCE_RANKS_SRC, SEQUENCE_RANKS_BIN, force, verbose)


SEQUENCE_PARTITION_SRC = os.path.join(REPO, "tests", "cpp", "sequence_partition_tests.cpp")
SEQUENCE_PARTITION_BIN = os.path.join(REPO, "tests", "cpp", "_build", "sequence_partition_tests")


def build_sequence_partition_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's sequence_partition / sequence_log_probs test program."""
    return _build_cpp_program(SEQUENCE_PARTITION_SRC, SEQUENCE_PARTITION_BIN, force, verbose)


ITEM_SET_SRC = os.path.join(REPO, "tests", "cpp", "item_set_tests.cpp")
ITEM_SET_BIN = os.path.join(REPO, "tests", "cpp", "_build", "item_set_tests")


def build_item_set_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's item-set test program."""
    return _build_cpp_program(ITEM_SET_SRC, ITEM_SET_BIN, force, verbose)


ROLLOUT_SRC = os.path.join(REPO, "tests", "cpp", "rollout_tests.cpp")
ROLLOUT_BIN = os.path.join(REPO, "tests", "cpp", "_build", "rollout_tests")


def build_rollout_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's rollout test program."""
    return _build_cpp_program(ROLLOUT_SRC, ROLLOUT_BIN, force, verbose)


BEAM_SRC = os.path.join(REPO, "tests", "cpp", "beam_tests.cpp")
BEAM_BIN = os.path.join(REPO, "tests", "cpp", "_build", "beam_tests")


def build_beam_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's beam-search test program."""
    return _build_cpp_program(BEAM_SRC, BEAM_BIN, force, verbose)


ITEM_SET_ROLLOUT_SRC = os.path.join(REPO, "tests", "cpp", "item_set_rollout_tests.cpp")
ITEM_SET_ROLLOUT_BIN = os.path.join(REPO, "tests", "cpp", "_build", "item_set_rollout_tests")


def build_item_set_rollout_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's rollout / beam-search within an item set test program."""
    return _build_cpp_program(ITEM_SET_ROLLOUT_SRC, ITEM_SET_ROLLOUT_BIN, force, verbose)


RANK_ELIGIBLE_SRC = os.path.join(REPO, "tests", "cpp", "rank_eligible_tests.cpp")
RANK_ELIGIBLE_BIN = os.path.join(REPO, "tests", "cpp", "_build", "rank_eligible_tests")


def build_rank_eligible_tests(force: bool = False, verbose: bool = True) -> str:
    """g++ build of the C++ host layer's rank_targets under a filter / set / store test program."""
    return _build_cpp_program(RANK_ELIGIBLE_SRC, RANK_ELIGIBLE_BIN, force, verbose)


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
    print(build_facade_tests(force="--force" in sys.argv))
    print(build_recommend_tests(force="--force" in sys.argv))
    print(build_ranking_tests(force="--force" in sys.argv))
    print(build_similar_tests(force="--force" in sys.argv))
    print(build_diverse_tests(force="--force" in sys.argv))
    print(build_candidates_tests(force="--force" in sys.argv))
    print(build_sessions_tests(force="--force" in sys.argv))
    print(build_sessions_seen_tests(force="--force" in sys.argv))
    print(build_sessions_replay_tests(force="--force" in sys.argv))
    print(build_filtered_tests(force="--force" in sys.argv))
    print(build_audience_tests(force="--force" in sys.argv))
    print(build_sampled_tests(force="--force" in sys.argv))
    print(build_partition_tests(force="--force" in sys.argv))
    print(build_above_tests(force="--force" in sys.argv))
    print(build_top_tests(force="--force" in sys.argv))
    print(build_capped_tests(force="--force" in sys.argv))
    print(build_sequence_ranks_tests(force="--force" in sys.argv))
    print(build_sequence_partition_tests(force="--force" in sys.argv))
    print(build_item_set_tests(force="--force" in sys.argv))
    print(build_rollout_tests(force="--force" in sys.argv))
    print(build_beam_tests(force="--force" in sys.argv))
    print(build_item_set_rollout_tests(force="--force" in sys.argv))
    print(build_rank_eligible_tests(force="--force" in sys.argv))
