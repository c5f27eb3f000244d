"""crass_amd — MI355X-native (gfx950) engine for crass's DR search + read recruitment path.

The product is ``libcrass_hip.so`` (hand-written HIP kernels + C-ABI host engine, see
``include/crass_hip.h``); this package is the thin Python host layer used by tests, bench.py
and the multi-GPU driver.  There is no CPU fallback: importing works everywhere, but every
search entry point needs the compiled library and a GPU.
"""
from ._abi import LIB_PATH, SYMBOLS, load  # noqa: F401
from .engine import (ConsensusResult, CrassError, FastxFile, FastxIndex, PackedReads, SearchEngine, SearchGroup, default_params,  # noqa: F401
                     consensus, dr_slots, ksw_batch, smith_waterman_batch, merge_host, merge_rebuild, build_outputs, search_pipeline, search_pipeline_group, stream_fastx, synth_packed, synth_spec, unpack_ascii,
                     ResidentReads, Text, pack_code4, pack_layout, packed_arrays,
                     FastxDeclined, FastxLayout, fastx_header_ids, find_names, names_of, comments_of, fastx_scan_host,
                     FastxFilesDeclined, FastxFilesLayout, fastx_files_scan_host, FastxShards, fastx_files_shards_host, fastx_cut_probe_host,
                     BgzfDeclined, BgzfIndex, bgzf_index, bgzf_inflate_host, GzipPlan, gzip_inflate_host, GzipMembers, gzip_inflate_members_host, gzip_inflate_ranges_host, gzip_inflate_members_ranges_host, fastx_files_shards_host_gzip)

__all__ = ["ConsensusResult", "consensus", "ksw_batch", "smith_waterman_batch", "CrassError", "FastxFile", "FastxIndex", "PackedReads", "SearchEngine", "SearchGroup", "default_params", "search_pipeline", "search_pipeline_group", "merge_host", "merge_rebuild", "build_outputs", "dr_slots",
           "ResidentReads", "Text", "pack_code4", "pack_layout", "packed_arrays", "FastxDeclined", "FastxLayout", "fastx_header_ids", "find_names", "names_of", "comments_of", "fastx_scan_host", "FastxFilesDeclined", "FastxFilesLayout", "fastx_files_scan_host", "FastxShards", "fastx_files_shards_host", "fastx_cut_probe_host", "BgzfDeclined", "BgzfIndex", "bgzf_index", "bgzf_inflate_host", "GzipPlan", "gzip_inflate_host", "GzipMembers", "gzip_inflate_members_host", "gzip_inflate_ranges_host", "gzip_inflate_members_ranges_host", "fastx_files_shards_host_gzip", "stream_fastx", "synth_packed", "synth_spec", "unpack_ascii", "load", "LIB_PATH", "SYMBOLS"]
