"""Float64 reference and float32 emulation of ONE extracted clip (include/sy11.h, sy11_iq_extract; definition in sy11/data/extract.py and
DESIGN.md §4), written on top of tests/_ddc_ref.py: a clip at decimation D is the DDC with P = 1, Q = D, the table ``prototype(1, D)``
rounded to float32 (as the kernel reads it) and centre 16 D, over the outputs [m0, m0 + M); D = 1 is the DDC's pure mixer.
No scipy here (the GPU tests import this module)."""
import numpy as np

from tests import _ddc_ref as R


def table(D):
    """-> (float32 (1, T) table, c) of decimation D >= 2, from the project's own prototype."""
    from sy11.data.resample import prototype
    h, c = prototype(1, D)
    return R.table_of(h.astype(np.float32), 1), c


def clip(x, D, dphi, m0, M, n0=0, f32=False):
    """Outputs [m0, m0 + M) of the clip grid of decimation D (output m = capture sample m D) of the capture whose samples
    [n0, n0 + len(x)) are ``x`` and that is zero elsewhere: float64, or with ``f32`` the kernel's arithmetic emulated in float32."""
    f = R.ddc_f32 if f32 else R.ddc_ref
    if D == 1:
        return f(x, None, 1, 1, 0, dphi, n0, m0, M)
    t, c = table(D)
    return f(x, t, 1, D, c, dphi, n0, m0, M)


def plan_clip(x, plan, k, n0=0, f32=False):
    """``clip`` for row ``k`` of an ``ExtractPlan``."""
    return clip(x, int(plan.D[k]), int(plan.dphi[k]), int(plan.m_first[k]), int(plan.M[k]), n0, f32)
