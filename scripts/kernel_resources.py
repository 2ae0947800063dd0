"""Per-kernel resources of one translation unit at two commits, from the compiler alone (no GPU).

    hipcc <the build's flags> -Rpass-analysis=kernel-resource-usage -c X.hip -o /dev/null 2> before.log     (at the parent)
    hipcc <the build's flags> --cuda-device-only -c X.hip -o before.co
    clang-offload-bundler --unbundle --type=o --input=before.co --targets=hip-amdgcn-amd-amdhsa--gfx950 --output=before.elf
    ... the same at this commit -> after.log, after.elf
    python scripts/kernel_resources.py before.log before.elf after.log after.elf

Prints, per kernel (demangled, the anonymous namespace dropped): SGPRs, VGPRs, AGPRs, private segment bytes/lane, occupancy
waves/SIMD, SGPR spills, VGPR spills, static LDS bytes (the compiler's remarks) and code bytes (the symbol's size in the
code object); `same` where parent and this commit agree on all nine, the two rows where they do not, and the kernels only
this commit has."""
import re
import subprocess
import sys

KEYS = ('TotalSGPRs', 'VGPRs', 'AGPRs', 'ScratchSize [bytes/lane]', 'Occupancy [waves/SIMD]', 'SGPRs Spill', 'VGPRs Spill',
        'LDS Size [bytes/block]')


def tool(name):
    import os
    import shutil
    return shutil.which(name) or os.path.join('/opt/rocm/llvm/bin', name)


def demangle(names):
    import shutil
    filt = shutil.which('llvm-cxxfilt') or shutil.which('c++filt')
    if filt is None:
        return list(names)
    out = subprocess.run([filt] + list(names), check=True, capture_output=True, text=True).stdout
    # (ddpg_rollout_kernel's argument type is a nest of std::conditional_t: written (...))
    # (the evaluation kernels' last template argument, SETS, came with the multi-set launches: a single-set
    # instantiation <.., false> keeps the name it had without it, so that it meets its row of the parent commit; the
    # SETS ones take a WithSets<...> argument: written (...))
    names = [re.sub(r'(ddpg_rollout_kernel<[^>]*>)\(.*\)$', r'\1(...)', s.replace('(anonymous namespace)::', ''))
             for s in out.splitlines()]
    names = [re.sub(r'((?:ppo|ddpg)_eval_kernel<[^>]*), false>', r'\1>', s) for s in names]
    names = [re.sub(r'std::conditional<false, WithSets<(\w+)>, \1>::type', r'\1', s) for s in names]
    return [re.sub(r'((?:ppo|ddpg)_eval_kernel<[^>]*, true>)\(.*\)$', r'\1(...)', s) for s in names]


def remarks(path):
    """{mangled name: [the eight remark figures]}"""
    kernels, cur = {}, None
    for line in open(path, errors='replace'):
        m = re.search(r'remark: Function Name: (\S+)', line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r'remark:\s+(.+?): (\S+) \[-Rpass-analysis', line)
        if m and cur is not None and m.group(1) in KEYS:
            cur[m.group(1)] = int(m.group(2))
    return {k: [v[key] for key in KEYS] for k, v in kernels.items()}


def code_bytes(elf):
    out = subprocess.run([tool('llvm-readelf'), '-sW', elf], check=True, capture_output=True, text=True).stdout
    sizes = {}
    for line in out.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == 'FUNC':
            sizes[f[7]] = int(f[2])
    return sizes


def table(log, elf):
    r, c = remarks(log), code_bytes(elf)
    names = sorted(r)
    return {d: r[m] + [c.get(m, -1)] for m, d in zip(names, demangle(names))}


def main():
    before, after = table(sys.argv[1], sys.argv[2]), table(sys.argv[3], sys.argv[4])
    row = lambda v: ' '.join(str(x) for x in v)  # noqa: E731
    old = sorted(k for k in after if k in before)
    print('## kernels of the parent commit (%d): parent -> this commit' % len(before))
    for k in sorted(before):
        if k not in after:
            print('gone    %s\n        %s' % (k, row(before[k])))
    for k in old:
        if before[k] == after[k]:
            print('same    %s\n        %s' % (k, row(after[k])))
        else:
            print('CHANGED %s\n        %s  ->  %s' % (k, row(before[k]), row(after[k])))
    new = sorted(k for k in after if k not in before)
    print('\n## new kernels (%d)' % len(new))
    for k in new:
        print('        %s\n        %s' % (k, row(after[k])))


if __name__ == '__main__':
    main()
