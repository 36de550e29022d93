"""`flashinfer.decode` as srt/layers/attention/flashinfer_backend.py takes it (:46, :1330, :1402, :1455): the decode wrapper and three host
helpers.  Nothing here launches a kernel."""
import torch

from .attention_wrappers import BatchDecodeWithPagedKVCacheWrapper  # noqa: F401


def _get_range_buf(seq_len: int, device):
    """int32 [0, 1, .., seq_len - 1] on `device` (the qo_indptr of a batch with one query token per request)"""
    return torch.arange(seq_len, dtype=torch.int32, device=device)


def get_seq_lens(kv_indptr, kv_last_page_len, page_size: int):
    """KV tokens per request from its page count and the fill of its last page; a request without pages has kv_last_page_len tokens"""
    return torch.clamp(kv_indptr[1:] - kv_indptr[:-1] - 1, min=0) * page_size + kv_last_page_len


def _grouped_size_compiled_for_decode_kernels(num_qo_heads: int, num_kv_heads: int) -> bool:
    """flashinfer <= 0.1.6: the group sizes its non-tensor-core decode kernels were compiled for (flashinfer_backend.py:1327-1338 picks
    `use_tensor_cores` from it; the MI355X kernel serves every group <= 16 on the matrix cores either way)"""
    return num_qo_heads // num_kv_heads in (1, 2, 4, 8)
