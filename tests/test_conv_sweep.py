"""The conv sweep's table against the launchers' sources, and its inputs against the bounds (no GPU).

* census: every clause of every `if (...) return 1;`, `return false;` and `return LTU_E_SHAPE;` of the conv launchers, split at
  its top-level `||`, is claimed by exactly one entry of RULES or UNSWEPT, by file, function and text; so is every
  `ltu_knob_pos(...)`; every claimed text still stands in its function.  Moving a threshold fails here until the sweep follows.
* sides: the shapes of a rule differ in the ruled quantity only, its clause is true on one and false on another, the refusal
  predicate agrees with the sides marked REFUSED, every shape is inside the size caps, every knob is a product knob.
* names: every kernel a side expects is a __global__ of csrc.
* generator: random_cases is reproducible, inside the caps and the accepted space, and covers every op, stride and concat kind.
* bound: a float32 CPU convolution of every rule side and of every random case is inside the element-wise bounds the GPU tests
  assert, so a failure there is the kernel's, not the inputs'.
"""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import conv_sweep_common as S
from tests import test_gpu_conv_paths as CP

SEED, NRANDOM = 20261021, 240


# ---------------------------------------------------------------------------------------------- parsing the launchers
def _source(name):
    with open(os.path.join(CP.CSRC, name)) as f:
        return re.sub(r'//[^\n]*', '', f.read())


_DEF = re.compile(r'^(?![ \t#/}])(?:[\w:<>*&"]+[ \t]+)+\**(\w+)\s*\(', re.M)


def functions(src):
    """{name: text} of the column-0 definitions of a source (a definition's text runs to the next one)"""
    starts = [(m.start(), m.group(1)) for m in _DEF.finditer(src)]
    return {name: src[pos:(starts[i + 1][0] if i + 1 < len(starts) else len(src))] for i, (pos, name) in enumerate(starts)}


def _close(src, i):
    """index past the parenthesis that closes the one at src[i]"""
    depth = 0
    for j in range(i, len(src)):
        depth += {'(': 1, ')': -1}.get(src[j], 0)
        if depth == 0:
            return j + 1
    raise ValueError('unbalanced')


def _norm(text):
    return ' '.join(text.split())


def split_or(cond):
    """a condition at its top-level ||"""
    out, depth, last = [], 0, 0
    for i, ch in enumerate(cond):
        depth += {'(': 1, ')': -1}.get(ch, 0)
        if depth == 0 and cond.startswith('||', i):
            out.append(cond[last:i])
            last = i + 2
    return [_norm(c) for c in out + [cond[last:]]]


def census():
    """{(file, function, clause)} of the shape refusals and {(file, function, call)} of the ltu_knob_pos calls of the conv launchers"""
    clauses, knobs = set(), set()
    for name in S.CENSUS_FILES + [S.F_GEMM]:
        for fn, body in functions(_source(name)).items():
            if name == S.F_GEMM and fn not in S.CENSUS_GEMM:
                continue
            for m in re.finditer(r'\bif\s*\(', body):
                end = _close(body, m.end() - 1)
                if re.match(r'\s*return\s+(1|false|LTU_E_SHAPE)\s*;', body[end:]):
                    clauses.update((name, fn, c) for c in split_or(body[m.end():end - 1]))
            for m in re.finditer(r'\bltu_knob_pos\s*\(', body):
                knobs.add((name, fn, _norm(body[m.start():_close(body, m.end() - 1)])))
    return clauses, knobs


def claims():
    """[(file, function, text, claimant)] of RULES and UNSWEPT"""
    return ([(f, fn, _norm(t), r.name) for r in S.RULES for f, fn, t in r.sources]
            + [(f, fn, _norm(t), 'UNSWEPT') for f, fn, t, _ in S.UNSWEPT])


def test_split_or():
    assert split_or('a % 8 || (b || c) && d ||\n  f(x, y) >= (1LL << 31)') == ['a % 8', '(b || c) && d', 'f(x, y) >= (1LL << 31)']


def test_census_every_clause_is_claimed_once():
    clauses, knobs = census()
    assert len(clauses) > 100 and len(knobs) >= 12, (len(clauses), len(knobs))
    claimed = {}
    for f, fn, t, who in claims():
        claimed.setdefault((f, fn, t), []).append(who)
    twice = {k: v for k, v in claimed.items() if len(v) > 1}
    assert not twice, f'claimed more than once: {twice}'
    missing = sorted(c for c in clauses if c not in claimed)
    assert not missing, 'shape clauses of the launchers that neither RULES nor UNSWEPT claims:\n' + '\n'.join(map(str, missing))
    loose = sorted(k for k in knobs if not any(f == k[0] and fn == k[1] and k[2] in t for f, fn, t in claimed))
    assert not loose, 'ltu_knob_pos calls of the launchers that neither RULES nor UNSWEPT claims:\n' + '\n'.join(map(str, loose))


def test_census_every_claim_still_stands():
    bodies = {}
    gone = []
    for f, fn, t, who in claims():
        if f not in bodies:
            bodies[f] = {k: _norm(v) for k, v in functions(_source(f)).items()}
        if t not in bodies[f].get(fn, ''):
            gone.append((who, f, fn, t))
    assert not gone, 'claimed texts that no longer stand in their function:\n' + '\n'.join(map(str, gone))
    for r in S.RULES:
        assert r.sources, r.name


def test_unswept_reasons():
    for f, fn, t, why in S.UNSWEPT:
        assert len(why) > 40, (f, fn, t)


# ---------------------------------------------------------------------------------------------- the table itself
def _product_knobs():
    src = ''.join(open(os.path.join(CP.CSRC, n)).read() for n in sorted(os.listdir(CP.CSRC)) if n.endswith(('.hip', '.h')))
    src = re.sub(r'#ifdef LTU_EXPERIMENTS.*?#(?:else|endif)', '', src, flags=re.S)
    return set(re.findall(r'"(LTU_[A-Z0-9_]+)"', src))


def test_rule_names_are_unique():
    assert len({r.name for r in S.RULES}) == len(S.RULES)


@pytest.mark.parametrize('rule', S.RULES, ids=[r.name for r in S.RULES])
def test_sides(rule):
    dirs = (rule.direction,) if isinstance(rule.direction, str) else rule.direction
    assert rule.op in ('conv3d', 'pair', 'upconv') and set(dirs) <= {'fwd', 'dgrad', 'wgrad'} and rule.arg
    assert 2 <= len(rule.sides) <= 3
    assert set(rule.knobs) <= _product_knobs(), 'knobs must exist and be read outside LTU_EXPERIMENTS'
    truth = [bool(rule.clause(S.launcher_args(rule.op, dirs[0], sd.shape))) for sd in rule.sides]
    assert True in truth and False in truth, f'the clause must hold on one side and not on another: {truth}'
    first = rule.sides[0].shape
    for sd in rule.sides[1:]:
        diff = {k for k in first if first[k] != sd.shape[k]}
        assert diff and diff <= set(rule.varies), f'sides differ in {diff}, the rule varies {rule.varies}'
    for sd in rule.sides:
        assert S.out_voxels(rule.op, sd.shape) <= S.MAX_VOXELS and S.row_macs(rule.op, sd.shape) <= S.MAX_ROW_MACS
        why = S.refusal(rule.op, sd.shape, sd.backward)
        assert (why is not None) == (sd.kernels == S.REFUSED), f'{rule.case(sd).name}: refusal() says {why}, the side {sd.kernels}'
        if sd.kernels != S.REFUSED:
            assert set(sd.kernels) <= set(dirs) and sd.kernels, 'a side names kernels in the directions of its rule'
            assert sd.backward or set(sd.kernels) == {'fwd'}


def test_side_kernels_exist_in_sources():
    src = CP.csrc_text()
    names = {k for r in S.RULES for sd in r.sides if sd.kernels != S.REFUSED for ks in sd.kernels.values() for k in ks}
    assert len(names) >= 15
    for fn in sorted(names):
        assert '<' not in fn and CP.is_global(fn, src), f'{fn}: no __global__ {fn} in lintransunet_amd/csrc'


# ---------------------------------------------------------------------------------------------- the random fill
def test_random_cases():
    cases = S.random_cases(SEED, NRANDOM)
    again = S.random_cases(SEED, NRANDOM)
    assert [(c.name, c.shape) for c in cases] == [(c.name, c.shape) for c in again]
    assert [c.name for c in S.random_cases(SEED + 1, 12)] != [c.name for c in cases[:12]]
    assert len({c.name for c in cases}) == NRANDOM
    count = {}
    for c in cases:
        s = c.shape
        assert S.refusal(c.op, s, c.backward) is None, c.name
        assert S.out_voxels(c.op, s) <= S.MAX_VOXELS and S.row_macs(c.op, s) <= S.MAX_ROW_MACS
        assert 1 <= s['B'] <= 3 and 1 <= s['H'] <= 13 and 1 <= s['W'] <= 13 and 1 <= s['D'] <= 19
        keys = [c.op, c.kind]
        if c.op == 'conv3d':
            keys += [s['stride'], ('concat', s['stride']) if s['C1'] else None, ('cop', s['cop']) if s['cop'] else None]
            assert not s['C1'] or (s['Ci'] % 8 == 0 and s['C1'] % 8 == 0)
        elif c.op == 'pair':
            keys.append(('n1', s['n1']))
        for k in keys:
            count[k] = count.get(k, 0) + 1
    want = (['conv3d', 'pair', 'upconv'] + S.KINDS + S.STRIDES + [('concat', st) for st in S.STRIDES]
            + [('cop', v) for v in (8, 16, 32)] + [('n1', v) for v in (8, 16, 32)])
    few = {k: count.get(k, 0) for k in want if count.get(k, 0) < 10}
    assert not few, f'kinds with fewer than 10 of {NRANDOM} cases: {few}'
    # every concat split in steps of 8 of some channel count, N % 8 != 0, odd extents
    assert {c.shape['Co'] for c in cases if c.kind == 'conv3d_oddN'} == set(S.ODD_N)
    assert len({(c.shape['Ci'], c.shape['C1']) for c in cases if c.kind == 'conv3d_concat'}) >= 20


def test_refusal_predicate():
    ok = CP.conv(1, 16, 16, 3, 5, 9)
    assert S.refusal('conv3d', ok) is None
    for k, v in (('Ci', 12), ('Ci', 6), ('C1', 4), ('Co', 6), ('Co', 12), ('stride', (1, 3, 1)), ('Ci', 0)):
        assert S.refusal('conv3d', dict(ok, **{k: v})) is not None, (k, v)
    assert S.refusal('conv3d', dict(ok, Co=12), backward=False) is None
    assert S.refusal('conv3d', dict(ok, Co=5, cop=8)) is None
    assert S.refusal('pair', CP.pair(1, 16, 8, 3, 8, 3, 5, 9)) is None
    assert S.refusal('pair', CP.pair(1, 16, 12, 3, 8, 3, 5, 9)) is not None
    assert S.refusal('pair', CP.pair(1, 16, 8, 3, 6, 3, 5, 9)) is not None
    assert S.refusal('upconv', CP.up(1, 8, 8, 2, 5, 3)) is None
    assert S.refusal('upconv', CP.up(1, 4, 8, 2, 5, 3)) is not None and S.refusal('upconv', CP.up(1, 8, 12, 2, 5, 3)) is not None


# ---------------------------------------------------------------------------------------------- the inputs fit the bounds
def _round(t):
    return t.bfloat16().double()


def float32_outputs(case):
    """{output: (fp32 CPU result as the kernels store it, float64 reference)}: bf16 for outputs and data gradients, fp32 for the
    weight and bias gradients; on the operands of CP.reference"""
    r = CP.reference(case, S.case_seed(case.name))
    s = case.shape
    f = torch.float32
    out = {}
    if case.op == 'conv3d':
        leaves = [t.to(f).requires_grad_(True) for t in (r['x0'], r['x1'], r['w'], r['b']) if t is not None]
        xin = torch.cat(leaves[:2], 1) if s['C1'] else leaves[0]
        y = F.conv3d(xin, leaves[-2], leaves[-1], stride=s['stride'], padding=1)
        out['y'] = (_round(y.detach()), r['y'][0])
        if case.backward:
            y.backward(r['go'].to(f))
            out['dx0'] = (_round(leaves[0].grad), r['dx'][0])
            if s['C1']:
                out['dx1'] = (_round(leaves[1].grad), r['dx'][1])
            out['dw'], out['db'] = (leaves[-2].grad.double(), r['dw'][0]), (leaves[-1].grad.double(), r['db'][0])
    elif case.op == 'pair':
        x, wa, ba, wb, bb = (r[k].to(f).requires_grad_(True) for k in ('x', 'wa', 'ba', 'wb', 'bb'))
        ya, yb = F.conv3d(x, wa, ba, padding=1), F.conv3d(x, wb, bb, padding=1)
        torch.autograd.backward([ya, yb], [r['ga'].to(f), r['gb'].to(f)])
        out.update(y0=(_round(ya.detach()), r['y'][0]), y1=(_round(yb.detach()), r['y'][1]), dx=(_round(x.grad), r['dx'][0]),
                   dwa=(wa.grad.double(), r['dw'][0]), dba=(ba.grad.double(), r['db'][0]),
                   dwb=(wb.grad.double(), r['dw'][1]), dbb=(bb.grad.double(), r['db'][1]))
    else:
        x = r['x'].to(f).requires_grad_(True)
        y = CP._upconv_classes(x, r['weff'].to(f), r['b'].to(f))
        y.backward(r['go'].to(f))
        w, b = r['w'].to(f).requires_grad_(True), r['b'].to(f).requires_grad_(True)
        F.conv3d(F.interpolate(r['x'].to(f), scale_factor=2), w, b, padding=1).backward(r['go'].to(f))
        out.update(y=(_round(y.detach()), r['y'][0]), dx=(_round(x.grad), r['dx'][0]), dw=(w.grad.double(), r['dw'][0]),
                   db=(b.grad.double(), r['db'][0]))
    CP._REF.pop(case.name, None)
    return out


def fits_bounds(case):
    """worst error / bound of the float32 convolution per output; raises where one is outside"""
    worst = {}
    for k, (got, ref) in float32_outputs(case).items():
        worst[k] = CP.check_f32(k, got, ref) if k.startswith('d') and not k.startswith('dx') else CP.check_bf16(k, got, ref)
    return worst


@pytest.mark.parametrize('rule', S.RULES, ids=[r.name for r in S.RULES])
def test_rule_inputs_fit_the_bounds(rule):
    for sd in rule.sides:
        if sd.kernels != S.REFUSED:
            fits_bounds(rule.case(sd))


def test_random_inputs_fit_the_bounds():
    for case in S.random_cases(SEED, NRANDOM):
        fits_bounds(case)
