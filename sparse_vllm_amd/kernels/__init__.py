"""Python wrappers with the reference's kernel names/argument order
(src/sparsevllm/kernels/triton/*), each a thin call into libsvk.so."""

from .gqa_flash_decoding_stage1 import flash_decode_stage1, flash_decode_stage1_with_score  # noqa: F401
from .flash_decoding_stage2 import flash_decode_stage2  # noqa: F401
from .store_kvcache import store_kvcache  # noqa: F401
from .rkv_ops import redundancy_scores_from_slots, select_rkv_indices_batch  # noqa: F401
from .mla import (allocate_mla_decode_workspace, copy_latent_to_cache, decode_stage1, decode_stage2,  # noqa: F401
                  gather_latent_history, run_mla_decode, run_mla_prefill)
