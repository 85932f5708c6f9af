"""Proof that a source-only refactor of lintransunet_amd/csrc left the device code alone: every file of the Makefile's SRCS is
compiled to gfx950 assembly from two source trees with the Makefile's own flags (plain and with -DLTU_EXPERIMENTS), and each pair
is compared line by line.  Only what a rename of the zero line may change is normalised away: the zero-line symbol names
(ltu_zero_* and gemm_ring's former ring_zero_f32, with or without the _ZL<n> of internal linkage), the __hip_cuid_<hash> symbol,
and the data-section lines that define the zero line itself (.bss / .comm / .zero / .size / .addrsig_sym: its size and linkage may
differ).  Kernel bodies and every .amdhsa_* descriptor line must match exactly.
    python tools/asm_same.py OLD_TREE NEW_TREE [-j JOBS] [--keep DIR]
prints one verdict per file and build, exits 1 if any pair differs (the first differing lines are shown)."""
import argparse, difflib, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

CSRC = 'lintransunet_amd/csrc'
ZERO = re.compile(r'\b(?:_ZL\d+)?(?:ltu_zero_[A-Za-z0-9]+|ring_zero_f32)\b')
CUID = re.compile(r'__hip_cuid_[0-9a-f]+')
# lines of the zero line's own definition, after its name has become ZERO_LINE
BSS = re.compile(r'^\s*\.section\s+\.bss\b')
ZERO_DEF = re.compile(r'^\s*(?:\.(?:protected|type|globl|local|comm|size|addrsig_sym)\s+ZERO_LINE\b.*|ZERO_LINE:.*)$')


def makefile(tree):
    text = open(os.path.join(tree, CSRC, 'Makefile')).read()
    var = lambda name: re.search(r'^%s\s*\??=\s*(.*)$' % name, text, flags=re.M).group(1).strip()
    flags = var('CXXFLAGS').replace('$(ARCH)', var('ARCH')).split()
    return var('HIPCC'), flags, var('SRCS').split()


def normalised(path):
    out, after_label = [], False
    for line in open(path).read().split('\n'):
        line = CUID.sub('__hip_cuid_X', ZERO.sub('ZERO_LINE', line))
        # a zero line with external linkage opens .bss itself and __hip_cuid_X follows in it; one with internal linkage is a .comm
        # and __hip_cuid_X opens .bss: the section line and the blank lines around the definitions carry no code
        if not line.strip() or BSS.match(line):
            continue
        if ZERO_DEF.match(line):
            after_label = line.startswith('ZERO_LINE:')
            if after_label and out and re.match(r'^\s*\.p2align\b', out[-1]):
                out.pop()
            continue
        if after_label and re.match(r'^\s*\.zero\s+\d+', line):
            after_label = False
            continue
        after_label = False
        out.append(line)
    return out


def compile_one(job):
    tree, hipcc, flags, src, extra, dst = job
    cmd = [hipcc] + flags + extra + ['--cuda-device-only', '-S', src, '-o', dst]
    r = subprocess.run(cmd, cwd=os.path.join(tree, CSRC), capture_output=True, text=True)
    return dst, r.returncode, r.stderr


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('old_tree')
    ap.add_argument('new_tree')
    ap.add_argument('-j', type=int, default=8)
    ap.add_argument('--keep', help='directory that keeps the .s files (default: a temporary one)')
    a = ap.parse_args()
    tmp = None
    if a.keep:
        os.makedirs(a.keep, exist_ok=True)
        root = os.path.abspath(a.keep)
    else:
        tmp = tempfile.TemporaryDirectory()
        root = tmp.name
    builds = [('plain', []), ('experiments', ['-DLTU_EXPERIMENTS'])]
    jobs = []
    new_srcs = makefile(a.new_tree)[2]
    for side, tree in (('old', a.old_tree), ('new', a.new_tree)):
        hipcc, flags, srcs = makefile(tree)
        if srcs != new_srcs:
            sys.exit('the two Makefiles list different SRCS')
        for bname, extra in builds:
            os.makedirs(os.path.join(root, side, bname), exist_ok=True)
            for s in srcs:
                jobs.append((os.path.abspath(tree), hipcc, flags, s, extra, os.path.join(root, side, bname, s[:-4] + '.s')))
    with ThreadPoolExecutor(a.j) as ex:
        for dst, rc, err in ex.map(compile_one, jobs):
            if rc:
                sys.exit('compiling %s failed:\n%s' % (dst, err))
    bad = 0
    for bname, _ in builds:
        for s in new_srcs:
            o, n = (normalised(os.path.join(root, side, bname, s[:-4] + '.s')) for side in ('old', 'new'))
            same = o == n
            print('%-12s %-24s %s  (%d lines)' % (bname, s, 'identical' if same else 'DIFFERENT', len(n)))
            if not same:
                bad += 1
                for l in list(difflib.unified_diff(o, n, 'old/' + s, 'new/' + s, lineterm='', n=1))[:40]:
                    print('    ' + l)
    print('%d of %d pairs differ' % (bad, len(builds) * len(new_srcs)))
    if tmp:
        tmp.cleanup()
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
