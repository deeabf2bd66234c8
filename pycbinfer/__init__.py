"""Drop-in alias: `import pycbinfer` resolves to the MI355X implementation in `cbinfer_amd`.

The reference's applications import `pycbinfer`, reach the classes as `pycbinfer.CBConv2d` and
`pycbinfer.conv2d.CBConv2d` (sceneLabeling/modelConverter.py:33, poseDetection/evalTools.py:91,101),
and its pickled models name `pycbinfer.conv2d.CBConv2d` / `CBPoolMax2d`; all of these resolve here.
"""
import sys

import cbinfer_amd
from cbinfer_amd import *            # noqa: F401,F403

# every module that holds a module type of the package (the `module` column of chain.PRODUCERS) and the two of the
# reference's function level, under the reference's name
for _m in dict.fromkeys([row[1] for row in cbinfer_amd.chain.PRODUCERS] + ['conv2d_cg', 'conv2d_fg']):
    sys.modules[__name__ + '.' + _m] = globals()[_m] = getattr(cbinfer_amd, _m)
del _m

__all__ = cbinfer_amd.__all__
