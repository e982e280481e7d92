// The hdfs3_crc_ctx itself (include/hdfs3_crc.h): the error slot, the table images, a ctx's life cycle
// and settings, and the device-memory helpers.
//
// Error convention mirrors libhdfs3's C API (src/client/Hdfs.cpp:75-80,243-327):
// no exception crosses extern "C"; failures return a negative errno code and
// leave a thread-local message (hdfs3_crc_last_error, cf. hdfsGetLastError at
// Hdfs.cpp:59,329).
#include "hdfs3_crc.h"

#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>

#include "crc32c_tables.h"
#include "ctx.h"

namespace hdfs3crc {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char *what) {
    const int code = e == hipErrorOutOfMemory ? -ENOMEM
                     : e == hipErrorInvalidValue ? -EINVAL
                     : e == hipErrorNoDevice || e == hipErrorInvalidDevice ? -ENODEV
                                                                           : -EIO;
    return fail(code, "%s: %s", what, hipGetErrorString(e));
}

// Per polynomial ([0] CRC32C, [1] CRC32): slice tables, then the fold image (kFoldWords
// matrix columns, then the 4 affine nibble-table sets for G = 8, 16, 32, 64 of the round
// kernel), built once per process.
constexpr size_t kFoldUploadBytes = sizeof(uint32_t) * kFoldImageWords;  // the device copy

struct HostImage {
    uint32_t t[kSlices][kTableEntries];
    uint32_t fold[kFoldImageWords];
};

const HostImage *host_images() {
    static HostImage img[2];
    static std::once_flag once;
    std::call_once(once, [] {
        const uint32_t polys[2] = {kPolyReflected, kPolyCrc32};
        for (int p = 0; p < 2; ++p) {
            build_slice_tables(img[p].t, polys[p]);
            build_fold_matrices(img[p].t[0], img[p].fold);
            for (int set = 0; set < 4; ++set) {
                uint32_t *nib = img[p].fold + kFoldAffineOff + set * kFoldNibbleWords;
                build_fold_nibbles_pre(img[p].t[0], img[p].fold, set, nib);
                build_fold_affine(img[p].t[0], set, nib);
            }
        }
    });
    return img;
}

uint64_t table_image_bytes() { return 2 * (sizeof(HostImage::t) + kFoldUploadBytes); }

void select_checksum_type(hdfs3_crc_ctx *ctx, int type) {
    const int i = type == HDFS3_CHECKSUM_TYPE_CRC32C ? 0 : 1;
    ctx->d_tables = ctx->d_tables_by[i];
    ctx->d_fold = ctx->d_fold_by[i];
    ctx->poly = i == 0 ? kPolyReflected : kPolyCrc32;
    ctx->checksum_type = type;
}

bool is_device_memory_of(hdfs3_crc_ctx *ctx, const void *p) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != ctx->device) {
        (void)hipGetLastError();  // a host pointer is the caller's mistake, not a fault of the GPU
        return false;
    }
    return true;
}

}  // namespace hdfs3crc

using namespace hdfs3crc;

extern "C" {

const char *hdfs3_crc_last_error(void) { return g_err; }

int hdfs3_crc_ctx_create(int device, hdfs3_crc_ctx **out) {
    if (!out) return fail(-EINVAL, "null out");
    *out = nullptr;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(-ENODEV, "device %d not present (%d visible)", device, ndev);
    hdfs3_crc_ctx *ctx = new (std::nothrow) hdfs3_crc_ctx();
    if (!ctx) return fail(-ENOMEM, "ctx allocation");
    ctx->device = device;
    DeviceGuard g(device);
    auto bail = [&](int rc) {
        hdfs3_crc_ctx_destroy(ctx);
        return rc;
    };
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
        return bail(fail(-EIO, "hipGetDeviceProperties(%d) failed", device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return bail(fail(-ENODEV, "device %d is %s; this build targets gfx950 (MI355X) only",
                         device, prop.gcnArchName));
    ctx->grid_cap = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess)
        return bail(fail(-EIO, "hipStreamCreate failed"));
    ctx->stream = ctx->own_stream;
    if (ctx->result.grow(sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess)
        return bail(fail(-ENOMEM, "device allocation for ctx failed"));
    const HostImage *img = host_images();
    for (int p = 0; p < 2; ++p) {
        if (hipMalloc(reinterpret_cast<void **>(&ctx->d_tables_by[p]), sizeof(img[p].t)) != hipSuccess ||
            hipMalloc(reinterpret_cast<void **>(&ctx->d_fold_by[p]), kFoldUploadBytes) != hipSuccess)
            return bail(fail(-ENOMEM, "device allocation for ctx failed"));
        if (hipMemcpy(ctx->d_tables_by[p], img[p].t, sizeof(img[p].t), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(ctx->d_fold_by[p], img[p].fold, kFoldUploadBytes, hipMemcpyHostToDevice) != hipSuccess)
            return bail(fail(-EIO, "table upload failed"));
    }
    select_checksum_type(ctx, HDFS3_CHECKSUM_TYPE_CRC32C);
    *out = ctx;
    return 0;
}

void hdfs3_crc_ctx_destroy(hdfs3_crc_ctx *ctx) {
    if (!ctx) return;
    DeviceGuard g(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (Slot &s : ctx->slot) {
        s.release();
        if (s.done) (void)hipEventDestroy(s.done);
    }
    for (PacketArena &a : ctx->arena_cache) a.release();
    ctx->arena_cache.clear();
    for (auto &st : ctx->seg_ring) {
        st.seg.release();
        if (st.done) (void)hipEventDestroy(st.done);
        if (st.copied) (void)hipEventDestroy(st.copied);
    }
    if (ctx->desc_stream) {
        (void)hipStreamSynchronize(ctx->desc_stream);
        (void)hipStreamDestroy(ctx->desc_stream);
    }
    ctx->words.release();
    ctx->pieces.release();
    ctx->compose.release();
    for (int p = 0; p < 2; ++p) {
        if (ctx->d_tables_by[p]) (void)hipFree(ctx->d_tables_by[p]);
        if (ctx->d_fold_by[p]) (void)hipFree(ctx->d_fold_by[p]);
    }
    ctx->result.release();
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

int hdfs3_crc_ctx_set_stream(hdfs3_crc_ctx *ctx, void *hip_stream) {
    if (!ctx) return fail(-EINVAL, "null ctx");
    DeviceGuard g(ctx->device);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->own_stream;
    return 0;
}

void *hdfs3_crc_ctx_get_stream(hdfs3_crc_ctx *ctx) { return ctx ? ctx->stream : nullptr; }

int hdfs3_crc_ctx_set_checksum_type(hdfs3_crc_ctx *ctx, int type) {
    if (!ctx) return fail(-EINVAL, "null ctx");
    if (type != HDFS3_CHECKSUM_TYPE_CRC32C && type != HDFS3_CHECKSUM_TYPE_CRC32)
        return fail(-EINVAL, "checksum type %d has no CRC polynomial", type);
    select_checksum_type(ctx, type);
    return 0;
}

int hdfs3_crc_ctx_get_checksum_type(hdfs3_crc_ctx *ctx) { return ctx ? ctx->checksum_type : -EINVAL; }

int hdfs3_crc_ctx_synchronize(hdfs3_crc_ctx *ctx) {
    if (!ctx) return fail(-EINVAL, "null ctx");
    DeviceGuard g(ctx->device);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

uint64_t hdfs3_crc_ctx_kernel_launches(hdfs3_crc_ctx *ctx) { return ctx ? ctx->launches.load() : 0; }

int hdfs3_dev_malloc(void **d_ptr, size_t bytes) {
    if (!d_ptr) return fail(-EINVAL, "null out");
    HIP_TRY(hipMalloc(d_ptr, bytes));
    return 0;
}

int hdfs3_dev_free(void *d_ptr) {
    HIP_TRY(hipFree(d_ptr));
    return 0;
}

int hdfs3_host_malloc_pinned(void **h_ptr, size_t bytes) {
    if (!h_ptr) return fail(-EINVAL, "null out");
    HIP_TRY(hipHostMalloc(h_ptr, bytes, hipHostMallocDefault));
    return 0;
}

int hdfs3_host_free_pinned(void *h_ptr) {
    HIP_TRY(hipHostFree(h_ptr));
    return 0;
}

int hdfs3_memcpy_h2d(hdfs3_crc_ctx *ctx, void *d_dst, const void *h_src, size_t bytes) {
    if (!ctx) return fail(-EINVAL, "null ctx");
    DeviceGuard g(ctx->device);
    HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int hdfs3_memcpy_d2h(hdfs3_crc_ctx *ctx, void *h_dst, const void *d_src, size_t bytes) {
    if (!ctx) return fail(-EINVAL, "null ctx");
    DeviceGuard g(ctx->device);
    HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int hdfs3_memset_dev(hdfs3_crc_ctx *ctx, void *d_dst, int value, size_t bytes) {
    if (!ctx) return fail(-EINVAL, "null ctx");
    DeviceGuard g(ctx->device);
    HIP_TRY(hipMemsetAsync(d_dst, value, bytes, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // extern "C"
