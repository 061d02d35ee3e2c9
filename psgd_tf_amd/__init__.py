"""psgd_tf_amd -- MI355X-native engine for the PSGD preconditioner hot path.

Contents (only what the hot path needs):
  csrc/                                            HIP kernels + the C ABI (include/psgd_hip.h)
  _lib.py                                          ctypes binding / in-tree build
  preconditioned_stochastic_gradient_descent.py    host-side mirror of the reference module
  kron.py                                          Kronecker dispatch + formats
  kron_optimizer.py                                class Kron
  splu_optimizer.py                                class SPLU
  dense_optimizer.py                               class Dense
  xmat.py                                          the X-shaped / diagonal preconditioner (psgd_xmat.hip) and class XMat
  kron_quad.py                                     the inverse-free Kron whitening update on symmetric factors (psgd_kron_quad.hip)
  kron_quad_x3.py                                  ... with its products on the bf16 matrix cores at fp32 grade (psgd_kron_quad_x3.hip)
  kron_quad_diag.py                                ... with one diagonal side, for embedding-scale layers (psgd_kron_qdiag.hip)
  kron_quad_nd.py                                  ... on order-3 tensors with three symmetric factors (psgd_kron_qnd.hip)
  kron_quad_nd_list.py                             ... on a list of them: grouped launches, a Gram split along K (psgd_kron_qtlist.hip)
  multi_tail.py                                    the multi-tensor (list) kernels of its step tail as functions
  sharded.py                                       row-sharded multi-GPU UVd (torch.distributed / RCCL)
"""
from . import preconditioned_stochastic_gradient_descent as psgd  # noqa: F401

__all__ = ["psgd"]
