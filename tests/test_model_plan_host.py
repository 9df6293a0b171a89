"""The C plan builders (pps_amd/csrc/model_plan.hpp, what pps_model_create
compiles) against their Python twin pps_amd.model.build_plan(), on a CPU:
tests/plan_dump.cpp prints the C plan as JSON and every field of every layer,
the parameter table, the output blob and the feature width must be equal.
(tests/test_gpu_native.py holds the two equal again on the device, through
pps_model_create.)"""
import json
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

MARKET = 'market1501'
FPN = ['MODEL.CONV_BODY', 'FPN_reid.add_fpn_ResNet50_conv5_body', 'FPN.FPN_ON', True]
# (yaml, KEY VALUE overrides): the committed configurations, Market with the
# FPN level, and variants that take the builders' other branches
CASES = {
    'market1501': (MARKET, []),
    'duke': ('duke', []),
    'cuhk03': ('cuhk03', []),
    'market_fpn': (MARKET, FPN),
    # a strip count outside the reference's table: equal strips; wider heads
    'strips6_dim256': (MARKET, ['REID.BPM_STRIP_NUM', 6, 'REID.BPM_DIM', 256]),
    # res5 strided: stride in res5_0's 1x1, 12-row map, the table scaled by 1/2
    'res5_stride2': (MARKET, ['RESNETS.RES5_STRIDE', 2]),
    # the stride on the 3x3 instead of the first 1x1
    'stride_3x3': (MARKET, ['RESNETS.STRIDE_1X1', False, 'RESNETS.RES5_STRIDE', 2]),
    # dilated res5 (no stride rule, pad = dilation), a table strip count, FPN at another width
    'dilated_strips7_fpn512': (MARKET, FPN + ['RESNETS.RES5_DILATION', 2, 'REID.BPM_STRIP_NUM', 7,
                                              'FPN.DIM', 512]),
    # another input height (the table does not apply), no normalize layer, average pooling
    'h256_plain': (MARKET, ['REID.SCALE', (64, 256), 'REID.BPM_STRIP_NUM', 4,
                            'REID.NORMALIZE_FEATURE', False, 'REID.MAX_AVE_FEATURE', False,
                            'RESNETS.WIDTH_PER_GROUP', 32]),
}

# PlanLayer's fields and the value a Python layer dict without the key stands for
LAYER_DEFAULTS = dict(op=None, name='', bn='', input='', output='', residual='', cin=0, cout=0,
                      k=1, stride=1, pad=0, dil=1, relu=0, max_ave=0, dim=0, dim_inner=0,
                      split=[], prefixes=[])
CONFIG_FIELDS = ('height', 'width', 'strip_num', 'bpm_dim', 'num_groups', 'width_per_group',
                 'stride_1x1', 'res5_stride', 'res5_dilation', 'fpn_on', 'fpn_dim', 'max_ave',
                 'normalize')


def _compiler():
    cands = [os.environ.get('CXX'), shutil.which('g++')]
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    cands += [os.path.join(os.path.dirname(hipcc), 'clang++'),
              os.path.join(rocm, 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'bin', 'clang++')]
    for c in cands:
        if c and (shutil.which(c) or os.path.isfile(c)):
            return c
    pytest.fail('no C++ compiler: set CXX, or install g++ or the ROCm clang++ beside hipcc')


@pytest.fixture(scope='module')
def plan_dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('plan_dump') / 'plan_dump')
    subprocess.check_call([_compiler(), '-std=c++17', '-O1', '-Wall',
                           os.path.join(ROOT, 'tests', 'plan_dump.cpp'), '-o', exe])
    return exe


def _python_plan(yaml, overrides):
    from pps_amd import config, model, native
    config.merge_cfg_from_file(os.path.join(ROOT, 'configs', yaml, 'pps_crm_triplet_R-50_1x.yaml'))
    config.merge_cfg_from_list(overrides)
    k = native.config_from_cfg()
    return model.build_plan(), [getattr(k, f) for f in CONFIG_FIELDS]


def _norm(v):
    if v is None:
        return ''
    if isinstance(v, bool):
        return int(v)
    if isinstance(v, (list, tuple)):
        return [_norm(x) for x in v]
    return v


@pytest.mark.parametrize('case', sorted(CASES))
def test_c_plan_equals_python_plan(plan_dump, case):
    want, ints = _python_plan(*CASES[case])
    got = json.loads(subprocess.check_output([plan_dump] + [str(i) for i in ints]))
    assert len(got['layers']) == len(want.layers)
    for i, (g, p) in enumerate(zip(got['layers'], want.layers)):
        assert set(g) == set(LAYER_DEFAULTS), (i, sorted(g))
        assert set(p) <= set(LAYER_DEFAULTS), (i, sorted(p))   # nothing in the twin goes unchecked
        for f, default in LAYER_DEFAULTS.items():
            assert g[f] == _norm(p.get(f, default)), (case, i, p.get('name'), f, g[f], p.get(f))
    assert got['params'] == {n: list(s) for n, s in want.params.items()}
    assert got['output'] == want.output
    assert got['feat_dim'] == want.feat_dim


def test_market_plan_size(plan_dump):
    """The figures the plan is known by: 57 layers and 451 parameters for the
    Market configuration, 58 and 457 with the FPN level."""
    for case, (nl, npar) in {'market1501': (57, 451), 'market_fpn': (58, 457)}.items():
        from pps_amd import config
        config.reset_cfg()
        _, ints = _python_plan(*CASES[case])
        got = json.loads(subprocess.check_output([plan_dump] + [str(i) for i in ints]))
        assert (len(got['layers']), len(got['params'])) == (nl, npar), case
