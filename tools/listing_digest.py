"""One line per kernel of every csrc/*.hip, from the gfx950 listings: a diff aid for changes that must not move generated code.

    python tools/listing_digest.py > digest.txt        (compiles every csrc/*.hip to a listing under /tmp)

Tab-separated: demangled kernel name, hash of its normalised instruction stream, .amdhsa_next_free_vgpr,
.amdhsa_next_free_sgpr, LDS bytes (.amdhsa_group_segment_fixed_size), private segment bytes, source file; sorted by name.
Normalised: comments and directives dropped, the .LBB<n>_<m> labels renumbered per kernel in order of appearance (the function
number <n> moves with a kernel's position in its file), everything else -- symbol names of pc-relative addresses included --
kept.  Two digests of the same kernel agree exactly when its instructions, registers and memory sizes agree; the tool prints,
it does not compare or judge."""
import hashlib, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from barrier_scan import ROOT, listing_of

FIELDS = ('.amdhsa_next_free_vgpr', '.amdhsa_next_free_sgpr', '.amdhsa_group_segment_fixed_size', '.amdhsa_private_segment_fixed_size')
LABEL = re.compile(r'\.LBB\d+_\d+')


def digest(path):
    """-> {mangled kernel name: [hash, vgpr, sgpr, lds, private]} of one listing."""
    lines = open(path).read().splitlines()
    res, kern = {}, None
    for raw in lines:                                   # the kernel descriptors: which symbols are kernels, and their resources
        t = raw.split()
        if t[:1] == ['.amdhsa_kernel']:
            kern = t[1]
            res[kern] = dict.fromkeys(FIELDS, '?')
        elif t[:1] == ['.end_amdhsa_kernel']:
            kern = None
        elif kern and t and t[0] in FIELDS:
            res[kern][t[0]] = ' '.join(t[1:])
    out, kern, stream, names = {}, None, [], {}
    for raw in lines:
        s = raw.split(';')[0].strip()
        if kern is None:
            if s.endswith(':') and s[:-1] in res:
                kern, stream, names = s[:-1], [], {}
            continue
        if s.startswith('.Lfunc_end'):
            out[kern] = [hashlib.sha256('\n'.join(stream).encode()).hexdigest()[:16]] + [res[kern][f] for f in FIELDS]
            kern = None
        elif s and (not s.startswith('.') or s.endswith(':')):
            stream.append(LABEL.sub(lambda m: names.setdefault(m.group(0), f'.L{len(names)}'), s))
    return out


def main():
    out = tempfile.mkdtemp(prefix='sq_isa_')
    files = sorted(f for f in os.listdir(os.path.join(ROOT, 'image-stitcher_amd', 'csrc')) if f.endswith('.hip'))
    with ThreadPoolExecutor(max_workers=4) as pool:
        listings = list(pool.map(lambda f: listing_of(f, out), files))
    rows = [(k, v, f) for f, lst in zip(files, listings) for k, v in digest(lst).items()]
    plain = subprocess.run(['c++filt'], input='\n'.join(k for k, _, _ in rows), capture_output=True, text=True).stdout.splitlines()
    for name, (_, v, f) in sorted(zip(plain, rows)):
        print('\t'.join([name] + v + [f]))


if __name__ == '__main__':
    main()
