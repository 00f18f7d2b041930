#!/usr/bin/env python
"""Tuning build: compile only SOME kernel translation units (the full library takes ~5.5 min on 8 cores) into
dgpmp2_amd/lib/libdgpmp2_dev.so; the launch entry points of the units left out are stubs that fail with hipErrorInvalidValue.
Use it with DGP_LIB_PATH=dgpmp2_amd/lib/libdgpmp2_dev.so (dgpmp2_amd/_capi.py).  Never the product build.

  python profiles/tools/devbuild.py 2_f32_g0 2_f32_g1 [-D...] [-o name.so]     units: <dof>_<f32|f64>_g<0 static|1 general|2 backward|3 per-state Kronecker|4 chain backward>
Prints the ISA statistics (registers, scratch, instruction counts) of the kernels whose name contains --show (default ',16,4,').
"""
import argparse
import json
import os
import shutil
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from dgpmp2_amd._build import isa_stats, pipeline
from dgpmp2_amd._build.units import UNITS

INST = {u.name[len('gn_inst_'):]: u for u in UNITS if u.launcher}      # 2_f32_g0, 2t_f64_g3, 2e_f32_g1, ...: the gn_inst units of the product, by their short names
ALL = sorted(INST)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('units', nargs='+')
  ap.add_argument('-D', action='append', default=[])
  ap.add_argument('--flag', action='append', default=[], help='extra hipcc argument, e.g. --flag=-mllvm --flag=-amdgpu-spill-sgpr-to-vgpr=false')
  ap.add_argument('-o', default='libdgpmp2_dev.so')
  ap.add_argument('--show', default=',16,4,')
  ap.add_argument('--raw', action='store_true', help='plain hipcc -c: no repair of the device assembly')
  a = ap.parse_args()
  for u in a.units: assert u in ALL, (u, ALL)
  work = os.path.join('/tmp', 'dgp_dev_' + a.o.replace('.', '_'))
  shutil.rmtree(work, ignore_errors=True); os.makedirs(work)
  hipcc = pipeline.hipcc_path()
  # the units asked for, and the ones every library needs: the long-trajectory kernels (small), the C-ABI, dgp_sdf_2d (the binding resolves every declared symbol)
  built = [INST[u] for u in a.units]
  jobs = [pipeline.unit_job(u, work, ['-D' + d for d in a.D] + a.flag) for u in built + [u for u in UNITS if not u.launcher]]
  stub = os.path.join(work, 'stubs.hip')
  with open(stub, 'w') as f:      # every launcher of the product that is not built here (the ABI's launch tables reference them all)
    f.write('#include "%s"\n' % os.path.join(pipeline.CSRC, 'gn_device.h'))
    for u in UNITS:
      if u.launcher and u not in built:
        f.write('hipError_t %s(const dgp_host::KernelChoice&, const dgp::GnParams&, const dgp::GnGradParams*, hipStream_t) { return hipErrorInvalidValue; }\n' % u.launcher)
  stubs = pipeline.Job('stubs', stub, (), os.path.join(work, 'stubs', 'stubs.o'))
  # every unit through the product's own compile pipeline (pipeline.compile_hip_unit: device assembly, the exec-join repair, assembler, bundler, host object);
  # --raw: plain hipcc -c -save-temps (the unrepaired compiler output, for the reproducer builds of profiles/r06_compiler_fault.md); the stubs have no device code to repair
  one = lambda j: pipeline.compile_job(hipcc, j, repair=not a.raw and j is not stubs)
  with ThreadPoolExecutor(max_workers=pipeline.pool_size(len(jobs) + 1)) as ex: res = list(ex.map(one, jobs + [stubs]))      # (raises on the first failed unit)
  for j, r in zip(jobs, res):
    if r and (r[0] or r[1]): print('%-28s exec-join repair: %d instruction(s) moved, %d finding(s) left' % (os.path.basename(j.out), r[0], r[1]))
  out = os.path.join(ROOT, 'dgpmp2_amd', 'lib', a.o)
  pipeline.link_shared(hipcc, jobs + [stubs], out)
  stats = {}
  for u in built:
    for fn in os.listdir(os.path.join(work, u.name)):
      if fn.endswith('gfx950.s'): stats.update(isa_stats.parse(os.path.join(work, u.name, fn)))
  json.dump(stats, open(out + '.stats.json', 'w'), indent=1, sort_keys=True)
  for k, v in sorted(stats.items()):
    if a.show in k:
      print('%-46s vgpr %3d agpr %3d scratch %4d occ %d valu %5d f64 %5d dpp %4d agprmov %4d lds %4d vmem %3d/%3d' % (
          k, v['vgpr'], v['agpr'], v['scratch_bytes_per_lane'], v['waves_per_simd'], v['valu'], v['fma_f64'] + v['mul_f64'] + v['add_f64'], v['dpp'],
          v['agpr_moves'], v['lds'], v['vmem_load'], v['vmem_store']))
  print('built', out)


if __name__ == '__main__':
  main()
