"""The device sampler (csrc/sampler.hip, namespace l2s) has ONE kernel per phase of its default form: the row kernels, which serve a single
sequence as one row and a batch as many.  Read off the built library's gfx950 code objects (symbol names only): the sampler's kernels are
exactly the list below -- each of the seven margin phases once, none of the single-sequence copies they replaced, and the kernels of the
A/B forms (L2_SAMPLER_CHAIN, L2_SAMPLER_SERIAL) and of the running-sums diagnostic."""
import re
from collections import Counter

import pytest

import code_objects

MARGIN_PHASES = ["scaled_max_rows_kernel", "exp_rows_kernel", "sample_margin_rows_kernel", "runs_total_rows_kernel", "sort_tile_wide_rows_kernel",
                 "sort_rank_rows_kernel", "topp_margin_rows_kernel"]
DELETED = ["scaled_max_kernel", "exp_kernel", "sample_margin_kernel", "runs_total_kernel", "sort_tile_wide_kernel", "sort_rank_kernel",
           "topp_margin_kernel"]
AB_FORMS = ["sample_kernel", "softmax_kernel", "topp_kernel", "sort_tile_kernel<Lb0>", "sort_tile_kernel<Lb1>", "runs_kernel<Lb0>", "runs_kernel<Lb1>",
            "normalise_runs_kernel", "chain_kernel<Li1>", "chain_kernel<Li2>", "chain_kernel<Li3>", "tile_sums_kernel", "prefix_kernel"]


def sampler_kernel(mangled):
    """'name' or 'name<template arguments>' of a kernel of namespace l2s, else None."""
    m = re.match(r"_ZN3l2s(\d+)", mangled)
    if not m:
        return None
    rest = mangled[m.end():]
    name, rest = rest[:int(m.group(1))], rest[int(m.group(1)):]
    t = re.match(r"I((?:L[a-z]\d+E)+)E", rest)
    return name + ("<" + ",".join(re.findall(r"(L[a-z]\d+)E", t.group(1))) + ">" if t else "")


@pytest.fixture(scope="module")
def sampler_kernels(tmp_path_factory):
    names = code_objects.kernel_names(tmp_path_factory.mktemp("co"))
    return Counter(k for k in map(sampler_kernel, names) if k)


def test_the_sampler_has_one_kernel_per_margin_phase(sampler_kernels):
    for k in MARGIN_PHASES:
        assert sampler_kernels[k] == 1, (k, sampler_kernels[k])
    for k in DELETED:
        assert sampler_kernels[k] == 0, k
    assert sorted(sampler_kernels.elements()) == sorted(MARGIN_PHASES + AB_FORMS)
