"""VGPRs / scratch / spills of every render_kernel instantiation in the built library (llvm-readelf on the code objects), then
the feature, filter, ray-query, radiance-query, path-step and path-advance kernels (feature_kernel, atrous_kernel, query_kernel,
radiance_kernel, step_kernel, advance_kernel, advance_scan_kernel, advance_gather_kernel, light_sample_kernel, light_pdf_kernel,
advance_direct_kernel, shadow_kernel, advance_direct_gather_kernel, radiance_direct_kernel, film_direct_kernel) by name with their static LDS as well."""
import os, re, subprocess, sys
so = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'raytracinginoneweekendincuda_amd', 'librtow_hip.so')
# The kernels listed by name: patterns of the mangled name whose groups (name, strict, world, mode -- those the kernel has) make the label
TRAITS = r'ILi(?P<strict>\d)ENS\d?_(?:6affine)?12_GLOBAL__N_16TraitsILi(?P<world>\d)E'
LANE_KERNELS = [
    r'(?P<name>feature_kernel|radiance_kernel|step_kernel|advance_kernel|advance_direct_kernel|shadow_kernel|radiance_direct_kernel|film_direct_kernel)' + TRAITS,
    r'(?P<name>query_kernel)' + TRAITS + r'.*?EELi(?P<mode>\d)EEEv',  # MODE 0 closest hit, 1 occlusion
    r'(?P<name>light_sample_kernel|light_pdf_kernel)ILi(?P<strict>\d)E',
    r'(?P<name>atrous_kernel|advance_scan_kernel|advance_gather_kernel|advance_direct_gather_kernel)',
]
data = open(so, 'rb').read()
idx = [m.start() for m in re.finditer(b'\x7fELF', data)]
rows = []
others = []
for i, st in enumerate(idx[1:]):
    end = idx[i + 2] if i + 2 < len(idx) else len(data)
    open('/tmp/kt.elf', 'wb').write(data[st:end])
    out = subprocess.run(['/opt/rocm/lib/llvm/bin/llvm-readelf', '--notes', '/tmp/kt.elf'], capture_output=True, text=True).stdout
    cur = {}
    for line in out.splitlines():
        line = line.strip()
        m = re.match(r'\.(name|private_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size):\s*(\S+)', line)
        if m: cur[m.group(1)] = m.group(2)
        if line.startswith('.wavefront_size'):
            n = cur.get('name', '')
            affine = ' affine' if '_6affine' in n else ''   # a unit compiled with the general affine chain step (render.hip RT_AFFINE)
            if 'rtow6moving' in n: affine += ' moving'    # its second pass, with the moving step as well (render.hip RT_MOVING)
            m = re.search(r'render_kernelILi(\d)ENS\d?_(?:6affine)?12_GLOBAL__N_1(8AdaptiveINS\d_)?6TraitsILi(\d)ELb(\d)ELb(\d)ELi(\d)ELb(\d)ELb(\d)ELb(\d)ELi(\d+)ELb(\d)ELb(\d)', n)
            if m:
                adaptive = m.group(2) is not None  # the Adaptive<> form of the instantiation (render.hip)
                strict, world, comp, rich, waves, media, batch, nested, block, fast, grouped = (int(x) for k, x in enumerate(m.groups()) if k != 1)
                rows.append((int(adaptive) + (2 if affine else 0) + (4 if 'moving' in affine else 0), world, comp, rich, media, batch, nested, fast, grouped, block, waves, 'strict' if strict else 'fast',
                             int(cur['vgpr_count']), int(cur['private_segment_fixed_size']), int(cur['vgpr_spill_count'])))
            for pattern in LANE_KERNELS:
                m = re.search(pattern, n)
                if not m: continue
                g = m.groupdict()
                name = g['name'] + (' world ' + g['world'] if g.get('world') else '')
                if g.get('mode'): name += ' occlusion' if int(g['mode']) else ' closest'
                if g.get('strict'): name += ' strict' if int(g['strict']) else ' fast'
                others.append((name + affine, int(cur['vgpr_count']), int(cur['private_segment_fixed_size']), int(cur['vgpr_spill_count']),
                               int(cur['group_segment_fixed_size'])))
            cur = {}
print("world comp rich media batch nested fast grouped block waves build vgpr scratchB spills")
for r in sorted(rows): print(*r[1:], *(['adaptive'] if r[0] & 1 else []), *(['affine'] if r[0] & 2 else []), *(['moving'] if r[0] & 4 else []))
if others:
    print("kernel vgpr scratchB spills ldsB")
    for r in sorted(others): print(*r)
