"""CPU: the process-wide switches of libslotformer_hip.so as a fresh process sees them -- defaults, what each SF_* variable selects, setter before
the first get, what the setters store -- and slotformer_amd/switches.py PROCESS against them.  Every case is a child process with every SF_* variable
of this one removed; the child loads the library with ctypes (no GPU is opened) and prints what its calls returned.  All children are started
together, once per session.  (SF_CONV_WS has no getter: its rule is asserted by tools/switches_tsan.cpp, a stand-alone program.)"""
import json
import os
import subprocess
import sys

import pytest

CHILD = r'''
import ctypes, json, sys
h = ctypes.CDLL(sys.argv[1])
h.sf_last_error_string.restype = ctypes.c_char_p
out = []
for op in json.loads(sys.argv[2]):
    rc = getattr(h, op[0])(*op[1:])
    out.append([rc, h.sf_last_error_string().decode()] if op[0] == 'sf_set_precision' and rc != 0 else rc)
print(json.dumps(out))
'''

NAMES = ['precision', 'layer_tok', 'seam_fused', 'ffn_rows64', 'conv_fp16x2', 'slot_attn_tile16', 'encode_fuse_next', 'slot_chain', 'slot_attn_planes',
         'pixel_tok']
BOOLEANS = NAMES[1:]
DEFAULTS = dict(zip(NAMES, [1, 0, 1, 0, 0, 1, 1, 0, 1, 1]))
GET_ALL = [['sf_get_' + n] for n in NAMES]
ENV_VARS = {'precision': 'SF_PRECISION', 'layer_tok': 'SF_LAYER_TOK', 'seam_fused': 'SF_SEAM_FUSED', 'conv_fp16x2': 'SF_CONV_FP16X2'}

# (variable, value, result): the table of values, then the rule behind each (first character; 'bf16' exactly)
ENV_VALUES = [('SF_PRECISION', 'f32', 0), ('SF_PRECISION', '0', 0), ('SF_PRECISION', 'bf16', 2), ('SF_PRECISION', 'bf16x3', 1), ('SF_PRECISION', '1', 1),
              ('SF_LAYER_TOK', '1', 1), ('SF_LAYER_TOK', '0', 0), ('SF_SEAM_FUSED', '0', 0), ('SF_SEAM_FUSED', '1', 1),
              ('SF_CONV_FP16X2', '1', 1), ('SF_CONV_FP16X2', '0', 0)]
ENV_RULES = [('SF_PRECISION', 'fp32', 0), ('SF_PRECISION', '02', 0), ('SF_PRECISION', 'bf16 ', 1), ('SF_PRECISION', 'BF16', 1), ('SF_PRECISION', '2', 1),
             ('SF_PRECISION', '', 1),
             ('SF_LAYER_TOK', '10', 1), ('SF_LAYER_TOK', 'on', 0), ('SF_LAYER_TOK', '01', 0), ('SF_LAYER_TOK', '', 0),
             ('SF_SEAM_FUSED', '01', 0), ('SF_SEAM_FUSED', 'off', 1), ('SF_SEAM_FUSED', '10', 1), ('SF_SEAM_FUSED', '', 1),
             ('SF_CONV_FP16X2', '1x', 1), ('SF_CONV_FP16X2', 'yes', 0), ('SF_CONV_FP16X2', '', 0)]


def _env_cases():
    """The (variable, value, result) rows packed into as few environments as hold one value per variable each."""
    envs = []
    for var, val, res in ENV_VALUES + ENV_RULES:
        e = next((e for e in envs if var not in e), None)
        if e is None:
            e = {}
            envs.append(e)
        e[var] = (val, res)
    return envs


def _cases():
    cases = {'defaults': ({}, GET_ALL)}
    for i, e in enumerate(_env_cases()):
        cases[f'env{i}'] = ({k: v for k, (v, _) in e.items()}, GET_ALL)
    # a setter called before the first get wins and the variable is never read
    cases['set_first'] = ({'SF_LAYER_TOK': '1', 'SF_SEAM_FUSED': '0', 'SF_PRECISION': 'f32', 'SF_CONV_FP16X2': '1'},
                          [['sf_set_layer_tok', 0], ['sf_set_seam_fused', 1], ['sf_set_precision', 2], ['sf_set_conv_fp16x2', 0]] + GET_ALL)
    ops = []
    for n in BOOLEANS:
        for v in (5, 0, -3, 0, 7):
            ops += [['sf_set_' + n, v], ['sf_get_' + n]]
    cases['booleans'] = ({}, ops)
    cases['precision'] = ({}, [['sf_set_precision', 3], ['sf_get_precision'], ['sf_set_precision', -1], ['sf_get_precision'], ['sf_set_precision', 2],
                               ['sf_get_precision'], ['sf_set_precision', 7], ['sf_get_precision'], ['sf_set_precision', 0], ['sf_get_precision'],
                               ['sf_set_precision', 1], ['sf_get_precision']])
    # the rejected set is no first read either: the variable still counts behind it
    cases['precision_env'] = ({'SF_PRECISION': 'bf16'}, [['sf_set_precision', 3], ['sf_get_precision']])
    return cases


@pytest.fixture(scope='session')
def children():
    from slotformer_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), _lib.LIB_PATH
    clean = {k: v for k, v in os.environ.items() if not k.startswith('SF_')}
    procs = {name: subprocess.Popen([sys.executable, '-c', CHILD, _lib.LIB_PATH, json.dumps(ops)], env=dict(clean, **env), stdout=subprocess.PIPE,
                                    stderr=subprocess.PIPE, text=True) for name, (env, ops) in _cases().items()}
    out = {}
    for name, p in procs.items():
        so, se = p.communicate(timeout=120)
        assert p.returncode == 0, (name, se)
        out[name] = json.loads(so)
    return out


def test_defaults(children):
    assert dict(zip(NAMES, children['defaults'])) == DEFAULTS


def test_environment_values_and_rules(children):
    envs = _env_cases()
    assert sum(len(e) for e in envs) == len(ENV_VALUES) + len(ENV_RULES)
    by_var = {v: k for k, v in ENV_VARS.items()}
    for i, e in enumerate(envs):
        got = dict(zip(NAMES, children[f'env{i}']))
        want = dict(DEFAULTS, **{by_var[var]: res for var, (_, res) in e.items()})
        assert got == want, (e, got)


def test_setter_before_first_get_wins(children):
    got = children['set_first']
    assert got[:4] == [0, 0, 0, 0]
    assert dict(zip(NAMES, got[4:])) == dict(DEFAULTS, layer_tok=0, seam_fused=1, precision=2, conv_fp16x2=0)


def test_boolean_setters_store_zero_or_one(children):
    got = children['booleans']
    assert len(got) == len(BOOLEANS) * 10
    for i, n in enumerate(BOOLEANS):
        assert got[10 * i:10 * i + 10] == [0, 1, 0, 0, 0, 1, 0, 0, 0, 1], n   # (set, get) x (5, 0, -3, 0, 7): every set returns 0


def test_set_precision_validates(children):
    got = children['precision']
    for bad, value in ((got[0], got[1]), (got[2], got[3])):
        assert bad[0] < 0 and 'invalid argument: precision mode must be 0 (f32), 1 (bf16x3) or 2 (bf16)' in bad[1]
        assert value == 1
    assert got[4:6] == [0, 2]
    assert got[6][0] < 0 and 'precision' in got[6][1] and got[7] == 2
    assert got[8:] == [0, 0, 0, 1]
    bad, value = children['precision_env']
    assert bad[0] < 0 and value == 2


def test_python_table_mirrors_the_library(children):
    """switches.PROCESS names exactly the sf_set_* / sf_get_* pairs of the ABI, with the defaults and the variables the children saw."""
    from slotformer_amd import _lib, switches
    abi = {s for s in _lib.SIGNATURES if s.startswith(('sf_set_', 'sf_get_'))}
    assert {s for row in switches.PROCESS.values() for s in row[:2]} == abi and len(abi) == 2 * len(switches.PROCESS)
    assert list(switches.PROCESS) == NAMES
    for name, (setter, getter, env, default, text) in switches.PROCESS.items():
        assert (setter, getter) == ('sf_set_' + name, 'sf_get_' + name) and len(text) > 10
        assert default == dict(zip(NAMES, children['defaults']))[name], name
        assert env == ENV_VARS.get(name), name
        assert env is None or env in switches.SWITCHES
    # ... and each variable moves its own getter: the first environment case sets all four away from their defaults
    first = _env_cases()[0]
    assert set(first) == set(ENV_VARS.values())
    moved = {n for n, v in zip(NAMES, children['env0']) if v != DEFAULTS[n]}
    assert moved == {n for n, (_, _, env, _, _) in switches.PROCESS.items() if env}
    assert switches.process_table().count('\n') == len(switches.PROCESS) + 1
