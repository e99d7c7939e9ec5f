"""Compare two device assembly files of one source kernel by kernel: is a restructured source still compiled to the same code?

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S -fuse-cuid=none <source>.hip -o head.s     (the same for the parent's source -> parent.s)
    python tools/compare_kernel_streams.py parent.s head.s

One source file of roreg_amd/csrc at a time (ot_flash.hip with the extra -mllvm flag its Makefile rule adds); -fuse-cuid=none keeps the two
files free of a per-compilation id, so that whole files can be compared byte for byte as well.

Per kernel (every `.amdhsa_kernel` of either file) it compares
  * the instruction stream: the lines between the kernel's label and its descriptor, without comments, assembler directives and blank
    lines; local labels (.LBB<function>_<n>, .Ltmp<n>, ...) are renumbered in the order of their first appearance inside the kernel, so a
    kernel that merely moved inside the file still compares equal, and label definitions stay in the stream (a branch target that moved
    is a difference);
  * the descriptor values that decide occupancy: VGPR, SGPR and AGPR counts, LDS size, scratch size (and the rest of the descriptor block).
It prints one line per kernel -- name, instruction count, identical or not -- and exits 1 if any kernel differs or exists in one file only.
Equality is all it looks at: it knows no instruction by name."""
import re
import subprocess
import sys

_LABEL = re.compile(r'\.L[A-Za-z_]+\d+(?:_\d+)?')
_COUNTS = ('num_vgpr', 'num_agpr', 'numbered_sgpr', 'private_seg_size')


def kernels(path):
    """-> {kernel symbol: (instruction lines, descriptor lines)}"""
    lines = open(path).read().split('\n')
    out = {}
    for i, line in enumerate(lines):
        m = re.match(r'\s*\.amdhsa_kernel\s+(\S+)', line)
        if not m:
            continue
        name = m.group(1)
        start = max(k for k in range(i) if lines[k].startswith(name + ':'))
        labels = {}
        renumber = lambda mm: labels.setdefault(mm.group(0), f'.L{len(labels)}')
        stream = []
        for raw in lines[start + 1:i]:
            text = raw.split(';')[0].strip()
            if not text or (text.startswith('.') and not text.endswith(':')):
                continue                                   # comment, blank line or directive
            stream.append(_LABEL.sub(renumber, text))
        end = next(k for k in range(i, len(lines)) if lines[k].strip() == '.end_amdhsa_kernel')
        desc = [d.strip() for d in lines[i + 1:end]]
        for key in _COUNTS:
            desc += [d.strip().replace(name, '<kernel>') for d in lines if d.strip().startswith(f'.set {name}.{key},')]
        out[name] = (stream, desc)
    return out


def demangle(names):
    try:
        r = subprocess.run(['c++filt'], input='\n'.join(names), stdout=subprocess.PIPE, text=True, check=True)
        return dict(zip(names, r.stdout.split('\n')))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = sorted(set(a) | set(b))
    pretty = demangle(names)
    differ = 0
    for n in names:
        if n not in a or n not in b:
            verdict = f'ONLY IN {sys.argv[1] if n in a else sys.argv[2]}'
        else:
            same_stream, same_desc = a[n][0] == b[n][0], a[n][1] == b[n][1]
            verdict = 'identical' if same_stream and same_desc else 'DIFFERS (' + ', '.join(w for w, s in (('stream', same_stream), ('descriptor', same_desc)) if not s) + ')'
            if not same_stream:
                k = next((i for i, (x, y) in enumerate(zip(a[n][0], b[n][0])) if x != y), min(len(a[n][0]), len(b[n][0])))
                verdict += f' first at instruction {k}, {len(b[n][0])} instructions in the second file'
        differ += verdict != 'identical'
        print(f'{pretty[n]}: {len(a[n][0]) if n in a else len(b[n][0])} instructions, {verdict}')
    print(f'{len(names)} kernels, {differ} differ')
    sys.exit(1 if differ else 0)


if __name__ == '__main__':
    main()
