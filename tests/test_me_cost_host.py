"""CPU: odhip_me_search2 / odhip_me_costs2 / odhip_pipe_set_motion_search2 refuse bad jobs on the host, before any
HIP call (there is no GPU here), and the ctypes mirror of odhip_me_job2 has the library's size."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -10
W, H, PW, PH, F = 128, 64, 119, 55, 2
FAKE = 0x10000           # a non-NULL address: a refused job is never dereferenced


@pytest.fixture(scope="module")
def api():
    from daala_amd import build
    build.build()
    import daala_amd
    return daala_amd


def job2(D, flags=3, geom=1, **kw):
    """A job that passes every check for chroma planes of decimation `geom`, then the fields of kw."""
    cdec = geom
    refs = (ctypes.c_void_p * 3)(FAKE, FAKE, None)
    luma = D.MeJob(W, H, PW, PH, F, 2, 1, 3, 0, 5, PW, W, PW*PH, W*H, FAKE, refs, FAKE, FAKE)
    cw, ch = (PW + cdec) >> cdec, (PH + cdec) >> cdec
    j = D.MeJob2(luma=luma, flags=flags, cdec=cdec, lambda_subpel=3, reserved=0, csrc_stride=cw, cref_stride=W >> cdec,
                 csrc_plane_stride=cw*ch, cref_plane_stride=(W >> cdec)*(H >> cdec), csrc=FAKE,
                 cref=(ctypes.c_void_p * 3)(FAKE, FAKE, None))
    for k, v in kw.items():
        if k.startswith("luma_"):
            setattr(j.luma, k[5:], v)
        else:
            setattr(j, k, v)
    return j


def test_sizeof_matches_the_mirror(api):
    L = api.lib()
    assert L.odhip_me_sizeof(2) == ctypes.sizeof(api.MeJob2) == ctypes.sizeof(api.MeJob) + 72
    assert L.odhip_me_sizeof(0) == ctypes.sizeof(api.MeJob) and L.odhip_me_sizeof(3) == 0
    hdr = open(os.path.join(ROOT, "include", "daala_hip.h")).read()
    assert re.search(r"#define ODHIP_ME_CHROMA 1\b", hdr) and re.search(r"#define ODHIP_ME_SATD +2\b", hdr)
    assert (api.ME_CHROMA, api.ME_SATD) == (1, 2)


def test_bad_jobs_are_refused_on_the_host(api):
    L = api.lib()

    def search(j):
        return L.odhip_me_search2(ctypes.byref(j), None)

    def costs(j, n=1, c=FAKE, out=FAKE, metric=0):
        return L.odhip_me_costs2(ctypes.byref(j), ctypes.c_void_p(c), ctypes.c_long(n), metric, ctypes.c_void_p(out), None)

    no_cref1 = (ctypes.c_void_p * 3)(FAKE, None, None)
    for cdec in (0, 1):
        cw, ch = (PW + cdec) >> cdec, (PH + cdec) >> cdec
        bad = [dict(flags=4), dict(flags=-1), dict(flags=3 | 8), dict(cdec=-1), dict(cdec=2), dict(lambda_subpel=-1),
               dict(lambda_subpel=(1 << 20) + 1), dict(csrc=None), dict(cref=no_cref1), dict(csrc_stride=cw - 1),
               dict(cref_stride=(W >> cdec) - 1), dict(csrc_plane_stride=cw*ch - 1),
               dict(cref_plane_stride=(W >> cdec)*(H >> cdec) - 1),
               # everything odhip_me_search refuses
               dict(luma_coded_w=120), dict(luma_pic_w=W + 1), dict(luma_npics=0), dict(luma_nrefs=4),
               dict(luma_log_size=4), dict(luma_src_stride=PW - 1), dict(luma_ref_plane_stride=W*H - 1),
               dict(luma_src=None)]
        for kw in bad:
            assert search(job2(api, geom=cdec, **kw)) == EINVAL, (cdec, kw)
            assert costs(job2(api, geom=cdec, **kw)) == EINVAL, (cdec, kw)
        for kw in (dict(luma_range=-1), dict(luma_range=33), dict(luma_res=4), dict(luma_lambda_=-1),
                   dict(luma_lambda_=(1 << 20) + 1), dict(luma_grid=None)):
            assert search(job2(api, geom=cdec, **kw)) == EINVAL, (cdec, kw)
    # 4:2:0 strides are too small for 4:4:4 planes
    assert search(job2(api, geom=1, cdec=0)) == EINVAL
    # the chroma half is not looked at without the flag: only the flag-independent checks refuse such a job
    assert search(job2(api, flags=2, csrc=None, csrc_stride=0, lambda_subpel=-1)) == EINVAL
    assert search(job2(api, flags=0, csrc=None, luma_range=40)) == EINVAL
    assert L.odhip_me_search2(None, None) == EINVAL and L.odhip_me_costs2(None, None, ctypes.c_long(0), 0, None, None) == EINVAL
    assert costs(job2(api), c=None) == EINVAL and costs(job2(api), out=None) == EINVAL and costs(job2(api), n=-1) == EINVAL
    assert costs(job2(api), metric=2) == EINVAL and costs(job2(api), metric=-1) == EINVAL


def test_the_pipe_entry_point_refuses_without_a_pipe(api):
    assert api.lib().odhip_pipe_set_motion_search2(None, 1, 3, 0, 0, 0, 0) == EINVAL
