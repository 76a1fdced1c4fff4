"""The table of stream-order cases (tests/golden/stream_cases.py) against the two headers: every entry point that takes a
``void* stream`` is driven by a case or excluded with a reason, every case names a mechanism and poisons an input (or says why it
cannot), every mechanism the host code has gets a case, every case has a scenario in tests/test_stream_order_gpu.py, and no decoy is
non-finite or a uniform outside [0, 1)."""
import os
import re

import numpy as np

from tests.golden import stream_cases as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stream_entry_points():
    """Names of the functions of both headers that declare a ``void* stream`` parameter."""
    names = []
    for header in ("infv_ltm.h", "infv_vqf.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)                  # (parameter comments inside a declaration included)
        for m in re.finditer(r"\b(?:int|int64_t)\s+(infv_\w+)\s*\(([^;{}]*?)\)\s*;", text, re.S):
            if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
                names.append(m.group(1))
    return names


def test_the_parser_finds_the_entry_points():
    names = stream_entry_points()
    assert len(names) == len(set(names))
    for known in ("infv_ltm_forward", "infv_ltm_consolidate", "infv_ltm_source_weights", "infv_ltm_sync", "infv_vqf_encode_video",
                  "infv_vqf_encode_frames", "infv_vqf_mean", "infv_vqf_layernorm_tokens", "infv_vqf_frame_cross_attention"):
        assert known in names, known
    for no_stream in ("infv_ltm_create", "infv_ltm_set_probs", "infv_ltm_set_bins", "infv_ltm_rng_fill_host", "infv_vqf_set_context_tap"):
        assert no_stream not in names, no_stream
    assert len(names) >= 40, names


def test_every_stream_entry_point_has_a_case_or_a_stated_exclusion():
    names = set(stream_entry_points())
    driven = {e for c in st.CASES for e in c.entries}
    assert driven <= names, f"cases name entry points the headers do not declare with a stream: {sorted(driven - names)}"
    assert set(st.EXCLUSIONS) <= names, sorted(set(st.EXCLUSIONS) - names)
    assert not driven & set(st.EXCLUSIONS), "an entry point is both driven and excluded"
    missing = names - driven - set(st.EXCLUSIONS)
    assert not missing, f"entry points with a stream argument that no case drives and no exclusion explains: {sorted(missing)}"
    assert all(len(reason) > 20 for reason in st.EXCLUSIONS.values())


def test_every_case_names_a_mechanism_and_every_mechanism_has_a_case():
    used = set()
    for c in st.CASES:
        assert c.mechanism in st.MECHANISMS, f"{c.name}: unknown mechanism {c.mechanism!r}"
        assert c.family in st.FAMILIES, c.name
        assert c.entries and c.shape, c.name
        used.add(c.mechanism)
    assert used == set(st.MECHANISMS), f"mechanisms without a case: {sorted(set(st.MECHANISMS) - used)}"
    assert set(st.REQUIRED_MECHANISMS) <= used


def test_every_case_poisons_an_input_or_says_why_not():
    for c in st.CASES:
        assert c.poisoned or len(c.unpoisoned) > 20, f"{c.name}: poisons nothing and gives no reason"
        assert c.delay_ms == 0 or 10 <= c.delay_ms <= 100, f"{c.name}: delays stay in the tens of milliseconds"
    no_delay = [c.name for c in st.CASES if c.delay_ms == 0]
    assert no_delay == ["ltm_fresh_handle_first_call"], no_delay            # (the delay cannot hold the null stream)


def test_case_names_are_unique_and_the_controls_are_cases():
    names = [c.name for c in st.CASES]
    assert len(names) == len(set(names))
    assert set(st.DETERMINISM_CONTROLS) == set(st.FAMILIES)
    for fam, name in st.DETERMINISM_CONTROLS.items():
        assert st.BY_NAME[name].family == fam
    assert {st.BY_NAME[n].family for n in st.MISORDER_CONTROLS} == {"ltm", "vqf", "dropin"}
    assert "infv_ltm_consolidate" in st.BY_NAME["ltm_consolidate_70"].entries and "70 chunks" in st.BY_NAME["ltm_consolidate_70"].shape
    assert "infv_vqf_encode_video" in st.BY_NAME["vqf_encode_video_6"].entries


def test_every_case_has_a_scenario_and_every_scenario_a_case():
    from tests import test_stream_order_gpu as gpu                          # (importing it touches no device)
    assert set(gpu.SCENARIOS) == set(st.BY_NAME), sorted(set(gpu.SCENARIOS) ^ set(st.BY_NAME))


def test_no_decoy_is_non_finite_and_decoy_uniforms_stay_in_the_unit_interval():
    arrays = st.smallest_decoys()
    assert len(arrays) > 50
    for name, a in arrays.items():
        a = np.asarray(a)
        if a.dtype.kind != "f":
            continue                                                        # (position_ids and the like)
        assert np.isfinite(a).all(), f"decoy {name} has a non-finite value"
    u = arrays["uniforms"]
    assert u.dtype == np.float64 and (u >= 0).all() and (u < 1).all()
    # a decoy is another draw, not the good values again
    assert not np.array_equal(st.tokens(2, 2, 2, 32, True), st.tokens(2, 2, 2, 32, False))
    assert not np.array_equal(st.uniforms(2, 1, 4, True), st.uniforms(2, 1, 4, False))
    assert not np.array_equal(st.vqf_weights(True)["llama_proj.weight"], st.vqf_weights(False)["llama_proj.weight"])
