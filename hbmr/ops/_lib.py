"""ctypes binding of ``hbmr/lib/libhbmr.so`` (the native HIP/C++ kernels).

PyTorch is imported first so its bundled ``libamdhip64.so.7`` is the HIP
runtime in the process; libhbmr.so names the same soname and therefore shares
that runtime (streams and device pointers are interchangeable with torch's).

On a machine with a GPU the library MUST load: a missing or stale build raises
instead of silently falling back to a PyTorch path.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import threading
from pathlib import Path

import torch  # noqa: F401  (must precede the dlopen below)

_LIB_PATH = Path(__file__).resolve().parent.parent / "lib" / "libhbmr.so"
_lock = threading.Lock()
_lib = None

c_void_p = ctypes.c_void_p
c_long = ctypes.c_long
c_int = ctypes.c_int
c_uint = ctypes.c_uint
c_uint64 = ctypes.c_uint64
c_double_p = ctypes.POINTER(ctypes.c_double)

_SIGS = {
    "hbmr_kmeans_assign_bf16": (c_int, [c_void_p, c_long, c_int, c_void_p, c_void_p, c_int,
                                        c_void_p, c_void_p, c_void_p]),
    "hbmr_kmeans_accum_bf16": (c_int, [c_void_p, c_long, c_int, c_void_p, c_int, c_void_p,
                                       c_void_p, c_int, c_void_p, c_long, c_int, c_void_p]),
    "hbmr_kmeans_accum_f32": (c_int, [c_void_p, c_long, c_int, c_void_p, c_int, c_void_p,
                                      c_void_p, c_int, c_void_p, c_long, c_int, c_void_p]),
    "hbmr_kmeans_assign_top3_bf16": (c_int, [c_void_p, c_long, c_int, c_void_p, c_void_p, c_int,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hbmr_kmeans_assign_top3_f16": (c_int, [c_void_p, c_long, c_int, c_void_p, c_void_p, c_int,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hbmr_kmeans_exact_prep": (c_int, [c_void_p, c_long, c_int, c_int, c_int, c_int, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p]),
    "hbmr_kmeans_assign_top3_q1_grouped": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int,
                                                   c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                                   c_void_p, c_void_p, c_void_p, c_int, c_int,
                                                   c_void_p, c_void_p, c_void_p, c_void_p,
                                                   c_void_p, c_long, c_void_p, c_void_p]),
    "hbmr_kmeans_bound_workspace_bytes": (c_long, [c_long, c_int, c_int]),
    "hbmr_kmeans_assign_top3_q1_bounded": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int,
                                                   c_void_p, c_void_p, c_int, c_void_p,
                                                   c_void_p, c_void_p, c_void_p, c_int, c_int,
                                                   c_void_p, c_void_p, c_void_p, c_void_p,
                                                   c_void_p, c_long, c_void_p,
                                                   c_void_p, c_void_p, c_void_p, c_void_p,
                                                   c_void_p, c_long, c_void_p, c_void_p]),
    "hbmr_kmeans_centroid_nbr": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                         c_void_p, c_void_p]),
    "hbmr_kmeans_image16": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hbmr_kmeans_image16_tiled": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "hbmr_kmeans_set_exact_kernel": (c_int, [c_int]),
    "hbmr_kmeans_get_exact_kernel": (c_int, []),
    "hbmr_kmeans_refine_f32": (c_int, [c_void_p, c_long, c_int, c_int, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                       c_void_p]),
    "hbmr_kmeans_refine_batch_bytes": (c_long, [c_int, c_void_p]),
    "hbmr_kmeans_assign_top3_grouped": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int,
                                                c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                                c_void_p, c_void_p, c_void_p]),
    "hbmr_kmeans_refine_batch_q1g": (c_int, [c_int, c_void_p, c_int, c_int, c_int, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_long, c_void_p, c_void_p]),
    "hbmr_kmeans_refine_batch_q1": (c_int, [c_int, c_void_p, c_int, c_int, c_int, c_int,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_long, c_int,
                                            c_void_p, c_void_p]),
    "hbmr_kmeans_refine_batch_finish": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int,
                                                c_int, c_void_p, c_int, c_int, c_void_p,
                                                c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                                c_int, c_void_p, c_long, c_void_p]),
    "hbmr_kmeans_accum_workspace_bytes": (c_long, [c_long, c_int]),
    "hbmr_kmeans_batch_workspace_bytes": (c_long, [c_long, c_int, c_int]),
    "hbmr_kmeans_map_batch": (c_int, [c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                      c_int, c_void_p, c_void_p, c_long, c_void_p, c_void_p,
                                      c_int, c_int, c_void_p]),
    "hbmr_kmeans_delta_workspace_bytes": (c_long, [c_long, c_int, c_int]),
    "hbmr_kmeans_delta_combine": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                                          c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_int,
                                          c_void_p, c_void_p, c_void_p, c_void_p]),
    "hbmr_kmeans_map_batch_delta": (c_int, [c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                            c_int, c_int, c_void_p, c_void_p, c_long, c_void_p,
                                            c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                            c_void_p]),
    "hbmr_kmeans_update": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hbmr_kmeans_padded_k": (c_int, [c_int]),
    "hbmr_kmeans_map_cpu_f32": (c_int, [c_void_p, c_long, c_int, c_void_p, c_int, c_void_p,
                                        c_void_p, c_void_p, c_double_p, c_int, c_int]),
    "hbmr_kmeans_map_cpu_f32_ex": (c_int, [c_void_p, c_long, c_int, c_void_p, c_int, c_void_p,
                                           c_void_p, c_void_p, c_double_p, c_int, c_int, c_int,
                                           c_void_p]),
    "hbmr_kmeans_padded_dim": (c_int, [c_int]),
    "hbmr_f32_to_bf16_pad": (c_int, [c_void_p, c_long, c_int, c_int, c_void_p, c_void_p]),
    # sort / shuffle (native/kernels/sort.hip)
    "hbmr_radix_sort_workspace_bytes": (c_long, [c_long]),
    "hbmr_radix_onesweep_workspace_bytes": (c_long, [c_long]),
    "hbmr_radix_onesweep_status_bytes": (c_long, [c_long]),
    "hbmr_radix_sort_keys_u64": (c_int, [c_void_p, c_void_p, c_long, c_int, c_int, c_void_p,
                                         c_long, c_void_p, c_long, c_void_p, c_void_p, c_int,
                                         c_void_p]),
    "hbmr_radix_sort_pairs_u64": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int,
                                          c_int, c_void_p, c_long, c_void_p]),
    "hbmr_teragen": (c_int, [c_long, c_long, c_void_p, c_void_p]),
    "hbmr_tera_keys": (c_int, [c_void_p, c_long, c_int, c_void_p, c_void_p, c_void_p]),
    "hbmr_gather_u64": (c_int, [c_void_p, c_void_p, c_long, c_void_p, c_void_p]),
    "hbmr_gather_records": (c_int, [c_void_p, c_void_p, c_long, c_int, c_void_p, c_void_p]),
    "hbmr_split_offsets": (c_int, [c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_int,
                                   c_void_p, c_void_p]),
    "hbmr_check_sorted": (c_int, [c_void_p, c_void_p, c_long, c_void_p, c_void_p]),
    "hbmr_tera_collect": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_long,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hbmr_tera_collect_slots": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_long,
                                        c_void_p, c_void_p, c_void_p]),
    "hbmr_gather_records_multi": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int,
                                          c_void_p, c_void_p]),
    "hbmr_tera_partition_workspace_bytes": (c_long, [c_long, c_int]),
    "hbmr_tera_collect_gid": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_long,
                                      c_int, c_uint64, c_uint, c_uint, c_int, c_void_p, c_void_p,
                                      c_void_p]),
    "hbmr_gather_records_gid": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_void_p]),
    "hbmr_tera_group_stats": (c_int, [c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p,
                                      c_void_p]),
    "hbmr_radix_set_onesweep_waves": (c_int, [c_int]),
    "hbmr_gather_set_unroll": (c_int, [c_int]),
    "hbmr_tera_tie_fix_scratch_bytes": (c_long, [c_long, c_int]),
    "hbmr_tera_tie_fix_records": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_int, c_uint64,
                                          c_uint, c_uint, c_int, c_void_p, c_void_p, c_void_p,
                                          c_long, c_void_p]),
    "hbmr_merge_path": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p,
                                c_long, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hbmr_tera_tie_fix": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p]),
    "hbmr_tera_partition": (c_int, [c_void_p, c_long, c_int, c_void_p, c_void_p, c_int, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long,
                                    c_void_p]),
    # text / WordCount (native/kernels/text.hip)
    "hbmr_wc_tiles": (c_long, [c_long]),
    "hbmr_wc_tokenize_count": (c_int, [c_void_p, c_long, c_void_p, c_void_p]),
    "hbmr_wc_tokenize_write": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hbmr_wc_insert": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_long, c_void_p,
                               c_void_p, c_long, c_void_p, c_void_p]),
    "hbmr_wc_compact": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_long, c_int, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hbmr_wc_pack": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p,
                             c_void_p]),
    # grep (native/kernels/grep.hip)
    "hbmr_grep_cand_count": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_int, c_int, c_int,
                                     c_int, c_void_p, c_void_p, c_void_p]),
    "hbmr_grep_cand_write": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_int, c_int, c_int,
                                     c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hbmr_grep_select_blocks": (c_long, [c_long]),
    "hbmr_grep_block_max": (c_int, [c_void_p, c_long, c_void_p, c_void_p]),
    "hbmr_grep_prefix_max": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_void_p]),
    "hbmr_grep_select_count": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p]),
    "hbmr_grep_select_write": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p,
                                       c_void_p, c_void_p]),
    "hbmr_span_insert": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_long, c_void_p,
                                 c_void_p, c_long, c_void_p, c_void_p]),
    "hbmr_span_compact": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hbmr_lines_count": (c_int, [c_void_p, c_long, c_void_p, c_void_p]),
    "hbmr_lines_write": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p]),
    # record sort (native/kernels/recsort.hip)
    "hbmr_recsort_hash_partition": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p,
                                            c_void_p]),
    "hbmr_recsort_round_keys": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int,
                                        c_void_p, c_void_p, c_void_p]),
    "hbmr_recsort_round_workspace_bytes": (c_long, [c_long]),
    "hbmr_recsort_round": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_long, c_int, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_long, c_void_p]),
    "hbmr_recsort_cuts": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p,
                                  c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "hbmr_recsort_chunk_bytes": (c_int, []),
    "hbmr_recsort_gather": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_long, c_long, c_void_p, c_void_p]),
    # record join (native/kernels/recjoin.hip)
    "hbmr_recjoin_heads": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p,
                                   c_void_p]),
    "hbmr_recjoin_set_two_level": (c_int, [c_int]),
    "hbmr_recjoin_rank": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p,
                                  c_void_p, c_void_p]),
    "hbmr_recjoin_expand": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_long, c_int, c_void_p, c_long, c_long,
                                    c_void_p, c_void_p, c_void_p, c_void_p]),
    "hbmr_recjoin_frames": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                    c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p]),
    "hbmr_recjoin_copy": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long,
                                  c_void_p, c_void_p]),
    # record validation (native/kernels/recvalidate.hip)
    "hbmr_recvalidate_digest": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p]),
    "hbmr_recvalidate_order": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p]),
    # record generator (native/kernels/recgen.hip)
    "hbmr_recgen_chunk_bytes": (c_int, []),
    "hbmr_recgen_lengths": (c_int, [c_uint64, c_long, c_long, c_int, c_uint, c_uint, c_uint,
                                    c_uint, c_void_p, c_int, c_void_p, c_void_p]),
    "hbmr_recgen_fill_bytes": (c_int, [c_uint64, c_long, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_long, c_long, c_void_p, c_void_p]),
    "hbmr_recgen_fill_text": (c_int, [c_uint64, c_long, c_long, c_uint, c_uint, c_uint, c_uint,
                                      c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p]),
    # int-pair text (native/kernels/intpair.hip)
    "hbmr_intpair_tiles": (c_long, [c_long]),
    "hbmr_intpair_blocks": (c_long, [c_long]),
    "hbmr_intpair_lines_count": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_void_p]),
    "hbmr_intpair_lines_write": (c_int, [c_void_p, c_long, c_void_p, c_long, c_void_p, c_void_p]),
    "hbmr_intpair_parse": (c_int, [c_void_p, c_long, c_void_p, c_long, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p]),
    "hbmr_intpair_compact": (c_int, [c_void_p, c_void_p, c_long, c_void_p, c_long, c_void_p,
                                     c_void_p]),
    "hbmr_intpair_partition": (c_int, [c_void_p, c_long, c_long, c_void_p, c_void_p]),
    "hbmr_intpair_lengths": (c_int, [c_void_p, c_long, c_void_p, c_void_p]),
    "hbmr_intpair_fill": (c_int, [c_void_p, c_void_p, c_long, c_void_p, c_void_p]),
    # word tables (native/kernels/wordtab.hip)
    "hbmr_wordtab_tile_bytes": (c_int, []),
    "hbmr_wordtab_partition": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_uint, c_int,
                                       c_void_p, c_void_p]),
    "hbmr_wordtab_lengths": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p]),
    "hbmr_wordtab_fill": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_long, c_long, c_void_p, c_void_p]),
    # Snappy decode (native/kernels/snappydec.hip)
    "hbmr_snappy_decode": (c_int, [c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p]),
    # compressed SequenceFile splits (native/kernels/seqblock.hip)
    "hbmr_seqblock_vint": (c_int, [c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p,
                                   c_void_p]),
    "hbmr_seqblock_index": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_long, c_int, c_void_p, c_void_p, c_void_p]),
    "hbmr_seqblock_assemble": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_long, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_long,
                                       c_void_p]),
    "hbmr_seqblock_heads": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_long, c_void_p, c_long, c_void_p]),
    # exact cover / Pentomino (native/kernels/exactcover.hip)
    "hbmr_exactcover_expand_count": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                             c_void_p, c_long, c_void_p, c_void_p]),
    "hbmr_exactcover_expand_write": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                             c_void_p, c_long, c_void_p, c_long, c_long, c_void_p,
                                             c_void_p]),
    "hbmr_exactcover_count_blocks": (c_int, [c_int, c_int, c_int, c_long]),
    "hbmr_exactcover_count": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                      c_long, c_long, c_void_p, c_void_p, c_void_p, c_void_p]),
    # PiEstimator (native/kernels/pi.hip)
    "hbmr_pi_halton": (c_int, [ctypes.c_longlong, ctypes.c_longlong, c_void_p, c_void_p]),
    # GEMM (native/kernels/gemm.hip)
    "hbmr_gemm_bf16_tn": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_long, c_long,
                                  ctypes.c_float, c_int, c_void_p]),
    "hbmr_gemm_set_kernel": (c_int, [c_int]),
    "hbmr_gemm_bf16_tn_ex": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_long, c_long,
                                     ctypes.c_float, c_int, c_void_p, c_void_p]),
}


class NativeLibraryError(RuntimeError):
    pass


def lib_path() -> Path:
    return _LIB_PATH


def available() -> bool:
    try:
        load()
        return True
    except NativeLibraryError:
        return False


def load():
    """Load (once) and return the ctypes handle, building in-tree if needed."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not _LIB_PATH.exists() and os.environ.get("HBMR_AUTOBUILD", "1") == "1":
            try:
                import importlib.util
                spec = importlib.util.spec_from_file_location(
                    "hbmr_native_build", _LIB_PATH.parent.parent.parent / "native" / "build.py")
                mod = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(mod)
                mod.build()
            except Exception as e:  # pragma: no cover - surfaced below
                raise NativeLibraryError(f"libhbmr.so missing and build failed: {e}") from e
        if not _LIB_PATH.exists():
            raise NativeLibraryError(f"native library not found at {_LIB_PATH}; run native/build.py")
        try:
            lib = ctypes.CDLL(str(_LIB_PATH), mode=ctypes.RTLD_GLOBAL)
        except OSError as e:
            raise NativeLibraryError(f"cannot load {_LIB_PATH}: {e}") from e
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed with native error code {rc}")


def ptr(t):
    """Device address of a tensor as an int (None stays None: a null pointer)."""
    return None if t is None else t.data_ptr()


def stream_handle(stream=None) -> int:
    """hipStream_t of the given (or current) torch stream as an int."""
    if stream is None:
        stream = torch.cuda.current_stream()
    return int(stream.cuda_stream)


def is_cuda(t_or_device) -> bool:
    """Whether a tensor lies on a GPU, or a device (or its name) is one."""
    return torch.device(getattr(t_or_device, "device", t_or_device)).type == "cuda"


def stream_ctx(stream, t=None):
    """Enters ``stream``; nothing for None (the caller's current stream), or
    for a ``t`` (tensor or device) that is not on a GPU: the twin's path."""
    if stream is not None and (t is None or is_cuda(t)):
        return torch.cuda.stream(stream)
    return contextlib.nullcontext()
