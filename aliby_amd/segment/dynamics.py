"""
Host wrapper of the HIP Cellpose dynamics (aliby_amd/csrc/dynamics.hip): network outputs -> labels, for images and volumes.

Plays the role of cellpose.dynamics.compute_masks inside `model.eval` (reference call site
src/aliby/segment/dispatch.py:208-215).  torch only provides the device buffers.
"""

from __future__ import annotations

import numpy as np
import torch

from aliby_amd.extraction.engine import _ptr

_workspaces: dict = {}


def _mark(label):
    from aliby_amd import trace  # (diagnostic marks of the launch thread: ALIBY_RUNNER_TRACE)

    trace.mark(label)


def _workspace(need, device):
    """The device's workspace, shared by the image and volume dynamics and grown to the largest need so far."""
    key = (str(device),)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def _masks(eng, group, entry, workspace_bytes, ndim, dP, cellprob, niter, params, return_endpoints):
    """dP float32 [F,ndim,*frame] (one flow component per axis of a frame), cellprob float32 [F,*frame] (device) ->
    (labels uint16 [F,*frame] device, counts[F], end points [F,ndim,*frame] if return_endpoints) through the library's
    `entry`(ctx, dP, cellprob, F, *frame, niter, *params, workspace, bytes, labels, counts, end points, stream)."""
    assert dP.dtype == torch.float32 and cellprob.dtype == torch.float32
    dP = dP.contiguous()
    cellprob = cellprob.contiguous()
    F, ncomp, *frame = dP.shape
    assert ncomp == ndim == len(frame) and tuple(cellprob.shape) == (F, *frame)
    labels = torch.empty((F, *frame), dtype=torch.uint16, device=dP.device)  # (cleared by the library)
    n = np.zeros(max(F, 1), np.int32)
    need = int(workspace_bytes(F, *frame))
    ws = _workspace(need, dP.device)
    pf = torch.zeros_like(dP) if return_endpoints else None
    eng.call(entry, _ptr(dP), _ptr(cellprob), F, *frame, int(niter), *params, _ptr(ws), need, _ptr(labels), _ptr(n), _ptr(pf), group=group)
    if return_endpoints:
        return labels, n[:F], pf
    return labels, n[:F]


def masks_from_flows(eng, dP, cellprob, niter=200, cellprob_threshold=0.0, flow_threshold=0.4, min_size=15,
                     max_size_fraction=0.4, return_endpoints=False):
    """dP float32 [F,2,Y,X], cellprob float32 [F,Y,X] (device) -> (labels uint16 [F,Y,X] device, counts[F])."""
    from aliby_amd import trace

    _mark("dynamics:call")
    trace.about_to_block()  # (the call below waits for everything queued so far: ~100 ms for a 64-position batch)
    params = (float(cellprob_threshold), float(flow_threshold if flow_threshold is not None else 0.0), int(min_size),
              float(max_size_fraction))
    out = _masks(eng, "dynamics", "aliby_masks_from_flows", eng.lib.aliby_masks_workspace_bytes, 2, dP, cellprob, niter,
                 params, return_endpoints)
    _mark("dynamics:returned")
    return out


def masks_from_flows_3d(eng, dP, cellprob, niter=200, cellprob_threshold=0.0, min_size=15, max_size_fraction=0.4,
                        return_endpoints=False):
    """dP float32 [F,3,Z,Y,X] (dZ,dY,dX), cellprob float32 [F,Z,Y,X] (device) -> (labels uint16 [F,Z,Y,X] device, counts[F]).
    cellpose's 3-D compute_masks; there is no flow-error QC in 3-D."""
    params = (float(cellprob_threshold), int(min_size), float(max_size_fraction))
    return _masks(eng, "dynamics3d", "aliby_masks_from_flows_3d", eng.lib.aliby_masks3d_workspace_bytes, 3, dP, cellprob,
                  niter, params, return_endpoints)
