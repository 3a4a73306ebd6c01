/* od_occupancy.cuh - how many wavefronts of a deciding search kernel a SIMD holds (round 6 experiment,
   profiles/r6_overlap.txt).

   The step runs two chains on two streams.  Workgroups of two kernels share a compute unit only when the
   second one's FIT next to the first one's (tools/ubench/coresidency.hip, profiles/r6_coresidency_ubench.txt):
   the dispatcher hands out a workgroup as soon as some CU has the wave slots, VGPRs and LDS for it, and a
   kernel whose workgroups fit nowhere waits until the other kernel's drain.  The searches are compiled for
   three or four wavefronts per SIMD at 168 / 128 VGPRs - 504 to 512 of the 512 registers of every SIMD lane
   (rocprofv3's VGPR column counts register PAIRS on gfx950: its 84 is 168) - so nothing of the other stream,
   not even a 16-register memset, starts before a search ends (profiles/r6_timeline_before.csv).

   ODHIP_SEARCH_OCC == 2 compiles every deciding search for TWO wavefronts per SIMD at 176 - 200 VGPRs
   (amdgpu_num_vgpr counts pairs too; OD_SEARCH_VGPR_FLOOR pins the lower end: 170 registers or fewer would
   admit a third wavefront), which leaves 112 registers per lane, six wave slots per SIMD and >= 64 KB of LDS:
   one workgroup of k_forward_pyramid64x2 (107 VGPRs, 53 KB) or several of the smaller filter + DCT kernels
   then DO run beside a search (the luma pyramid's wall time inside the step falls from 1.0 to 0.2 - 0.5 ms)
   - and the step gets SLOWER, 3.57 -> 4.00 ms: the searches lose 14 - 17 % at two wavefronts, and the
   "HBM-bound" kernels they now share SIMDs with are no free riders (they issue 0.48 G of the step's 1.7 G
   VALU wave-instructions).  The default therefore stays what rounds 3-5 shipped (0); 2 and 3 are kept for
   the A/B (python -m daala_amd.build --variant occ2 -DODHIP_SEARCH_OCC=2; tools/gpu_r6_variants.sh). */
#pragma once
#ifndef ODHIP_SEARCH_OCC
# define ODHIP_SEARCH_OCC 0
#endif
#if ODHIP_SEARCH_OCC == 2
# define OD_SEARCH_OCC_ATTR __attribute__((amdgpu_waves_per_eu(2), amdgpu_num_vgpr(100)))    /* (the attribute counts register PAIRS on gfx90a and later: 200) */
# define OD_SEARCH_VGPR_FLOOR() asm volatile("" ::: "v175")
#elif ODHIP_SEARCH_OCC == 3
/* three wavefronts of 129 - 136 registers: 104 left - every filter + DCT kernel but the luma pyramid (107) */
# define OD_SEARCH_OCC_ATTR __attribute__((amdgpu_waves_per_eu(3), amdgpu_num_vgpr(68)))
# define OD_SEARCH_VGPR_FLOOR() asm volatile("" ::: "v128")
#else      /* rounds 3-5: the with-reference searches at three wavefronts, the no-reference ones as they come (four) */
# define OD_SEARCH_OCC_ATTR __attribute__((amdgpu_waves_per_eu(3)))
# define OD_DECIDE_OCC_ATTR
# define OD_SEARCH_VGPR_FLOOR() ((void)0)
#endif
#ifndef OD_DECIDE_OCC_ATTR
# define OD_DECIDE_OCC_ATTR OD_SEARCH_OCC_ATTR
#endif
/* Independent wavefronts per search workgroup sharing one 1/sqrt table (with-reference searches). */
#ifndef ODHIP_SEARCH_WAVES
# define ODHIP_SEARCH_WAVES 1
#endif
/* k_refb_lean_pair (the with-reference 32-coefficient bands a lane pair per band, pvq_refbands.hip): 9.5 KB of LDS
   per wavefront beside the workgroup's 4 KB table, 128 VGPRs without scratch.  Eight independent wavefronts per
   workgroup (80 KB: two workgroups per CU) at four per SIMD beat two per workgroup at three per SIMD (132 VGPRs)
   in every run of the step, 3.46 against 3.51 ms (profiles/refb_pair32.txt). */
#ifndef ODHIP_PAIR_WAVES
# define ODHIP_PAIR_WAVES 8
#endif
#ifndef ODHIP_PAIR_OCC
# define ODHIP_PAIR_OCC 4          /* amdgpu_waves_per_eu of that kernel */
#endif
/* The with-reference 128-coefficient bands a lane GROUP per band (k_refb_lean_pair<32, 4> / <64, 2>, the same
   template).  ODHIP_GROUP128_LANES: the default build's form, 4 = a quad per band (16 bands and 10.75 KB of
   LDS per wavefront: twelve wavefronts, three per SIMD, and their workgroups' 4 KB tables fit a CU's 160 KB,
   sixteen do not; 168 VGPRs without scratch), 2 = a pair (32 bands, 21.5 KB: seven wavefronts per CU at the
   most whatever the registers, so it is compiled for two per SIMD).  ODHIP_GROUP128_WAVES / _OCC = wavefronts
   per workgroup and amdgpu_waves_per_eu of the quad form, ODHIP_GROUP128_PAIR_WAVES / _OCC of the pair form.
   Measured on the step (profiles/refb_group128.txt): the quad at four wavefronts per workgroup 3.18 - 3.23 ms,
   at twelve 3.23 - 3.25, at six 3.30 - 3.31, the pair 3.31 - 3.36 (the row kernel: 3.37 - 3.41); on another
   box four 3.26 - 3.27, two 3.28 - 3.30, three 3.31. */
#ifndef ODHIP_GROUP128_LANES
# define ODHIP_GROUP128_LANES 4
#endif
#ifndef ODHIP_GROUP128_WAVES
# define ODHIP_GROUP128_WAVES 4
#endif
#ifndef ODHIP_GROUP128_OCC
# define ODHIP_GROUP128_OCC 3
#endif
#ifndef ODHIP_GROUP128_PAIR_WAVES
# define ODHIP_GROUP128_PAIR_WAVES 6
#endif
#ifndef ODHIP_GROUP128_PAIR_OCC
# define ODHIP_GROUP128_PAIR_OCC 2
#endif
/* The occupancy attribute of k_refb_lean_pair<nl, s> (the arguments are template parameters). */
#ifndef OD_GROUP_OCC_ATTR
# if ODHIP_SEARCH_OCC == 0
#  define OD_GROUP_OCC_ATTR(nl, s) __attribute__((amdgpu_waves_per_eu( \
    (nl)*(s) == 32 ? ODHIP_PAIR_OCC : (s) == 4 ? ODHIP_GROUP128_OCC : ODHIP_GROUP128_PAIR_OCC)))
# else
#  define OD_GROUP_OCC_ATTR(nl, s) OD_SEARCH_OCC_ATTR
# endif
#endif
