# libarchive_amd/host/sources.mk -- the sources of libla_host.so, stated once: the Makefile beside this file builds the
# product from them, tests/mock_gpu/Makefile the same sources over the CPU stand-ins of the device ABI.
LIBSRC  = la_lz4_index.c la_gzip_index.c la_read_core.c la_format_tar.c la_format_zip.c la_filter_lz4.c la_filter_gzip.c la_filter_zstd.c la_filter_bzip2.c la_filter_xz.c la_filter_lzip.c la_filter_lzop.c la_bid_policy.c la_zstd_index.c la_hash_dropin.c la_write_filters.c la_write_zstd.c la_write_bzip2.c la_write_xz.c la_write_lzip.c la_write_lzop.c la_write_zip.c
# the uu read filter: in the product, and not in LIBSRC, because the shared stand-in library of the tests has no
# la_gpu_uu_decode (tests/mock_gpu/uu.mk adds the filter and its stand-in to a build of its own); the read core registers
# the filter through a weak reference, so a library without it loads
LIBSRC_UU = la_filter_uu.c
