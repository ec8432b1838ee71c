// idc_rccl.hip -- the RCCL weight broadcast of the C ABI (include/ideepcolor.h): librccl opened at the first call, one broadcast of the packed blob,
// the received bytes validated like any other device blob.  The only unit that reads the environment in the default library (IDC_RCCL_PATH).
// No link-time dependency on librccl.
#include <dlfcn.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "idc_engine.h"

extern "C" {

// ---------------------------------------------------------------------------------------------- RCCL weight broadcast
// SURVEY.md 8b's export list / 8e: one broadcast of the packed blob from `root` over xGMI, called by every rank's
// process with its own handle.  librccl is opened at the first call (the copy torch already loaded, if any, else
// /opt/rocm's) -- the library has no link-time dependency on it, single-GPU users never touch it.
struct IdcNcclId { char internal[128]; };                  // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128), passed by value
struct Rccl {
    void* lib = nullptr;
    std::string path;
    std::string tried;                   // every candidate that failed, for the error string
    bool beside_runtime = false;         // opened from the directory of the libamdhip64 this library is bound to
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, IdcNcclId, int) = nullptr;
    int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
static Rccl* rccl() {
    static Rccl r;
    static bool tried = false;
    if (!tried) {
        tried = true;
        // RCCL launches its kernels on OUR stream handle, so it has to be the copy bound to the SAME libamdhip64 this
        // library resolved (a process that imported torch after this library holds two HIP runtimes: torch's bundled
        // librccl belongs to the other one, and a stream handle of one runtime means nothing to the other).  The HIP
        // runtime we call is found with dladdr; the librccl that ships beside it is the one to open.
        Dl_info di;
        std::string dir;
        if (dladdr((const void*)&hipStreamSynchronize, &di) && di.dli_fname) {
            dir = di.dli_fname;
            const size_t sl = dir.rfind('/');
            dir = sl == std::string::npos ? std::string() : dir.substr(0, sl + 1);
        }
        auto try_open = [&](const std::string& nm, int flags) {
            if (r.lib) return;
            r.lib = dlopen(nm.c_str(), flags);
            if (r.lib) r.path = nm; else r.tried += (r.tried.empty() ? "" : ", ") + nm;
        };
        if (const char* forced = getenv("IDC_RCCL_PATH")) try_open(forced, RTLD_NOW | RTLD_LOCAL);      // explicit override wins
        if (!dir.empty()) {
            try_open(dir + "librccl.so.1", RTLD_NOW | RTLD_LOCAL);
            try_open(dir + "librccl.so", RTLD_NOW | RTLD_LOCAL);
            r.beside_runtime = r.lib != nullptr && r.path.compare(0, dir.size(), dir) == 0;
        }
        // Not beside the runtime (split packages, LD_LIBRARY_PATH installs -- ADVICE r3: this search had been dropped): the loader's
        // own resolution.  A librccl found this way binds to whichever libamdhip64 the loader gives IT; when that is the runtime this
        // library uses (one ROCm install on the library path: the normal case) everything is as above, and the path travels in every
        // error string so a mismatch is diagnosable.
        if (!r.lib) {
            const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
            for (const char* nm : names) try_open(nm, RTLD_NOW | RTLD_LOCAL);
        }
        if (r.lib) {
            r.GetUniqueId = (int (*)(void*))dlsym(r.lib, "ncclGetUniqueId");
            r.CommInitRank = (int (*)(void**, int, IdcNcclId, int))dlsym(r.lib, "ncclCommInitRank");
            r.Broadcast = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(r.lib, "ncclBroadcast");
            r.CommDestroy = (int (*)(void*))dlsym(r.lib, "ncclCommDestroy");
            r.GetErrorString = (const char* (*)(int))dlsym(r.lib, "ncclGetErrorString");
            if (!r.GetUniqueId || !r.CommInitRank || !r.Broadcast || !r.CommDestroy) { r.tried += " (" + r.path + ": nccl symbols missing)"; r.lib = nullptr; }
        }
    }
    return r.lib ? &r : nullptr;
}
static std::string rccl_where() {            // for error strings: which librccl, and whether it is the runtime's sibling
    Rccl* r = rccl();
    if (!r) {
        static Rccl dummy;
        (void)dummy;
        return "librccl.so could not be opened (IDC_RCCL_PATH overrides the search)";
    }
    return r->path + (r->beside_runtime ? "" : " [not beside the libamdhip64 this library is bound to]");
}

int idc_comm_unique_id(void* id128) {
    if (!id128) return fail(nullptr, IDC_ERR_INVALID_ARG, "null id buffer");
    Rccl* r = rccl();
    if (!r) return fail(nullptr, IDC_ERR_UNSUPPORTED, "%s", rccl_where().c_str());
    const int e = r->GetUniqueId(id128);
    if (e != 0) return fail(nullptr, IDC_ERR_HIP, "ncclGetUniqueId failed: %s (%s)", r->GetErrorString ? r->GetErrorString(e) : "?", rccl_where().c_str());
    return IDC_OK;
}

int idc_broadcast_weights(idc_handle h, const void* unique_id, int rank, int world, int root) {
    if (!h || !unique_id) return fail(h ? &h->err : nullptr, IDC_ERR_INVALID_ARG, "null handle / id");
    if (world < 1 || rank < 0 || rank >= world || root < 0 || root >= world)
        return fail(&h->err, IDC_ERR_INVALID_ARG, "rank %d / root %d outside world %d", rank, root, world);
    if (rank == root && !h->weights_set) return fail(&h->err, IDC_ERR_NO_WEIGHTS, "the root rank has no weights to broadcast");
    Rccl* r = rccl();
    if (!r) return fail(&h->err, IDC_ERR_UNSUPPORTED, "%s", rccl_where().c_str());
    HIPCHK(h, hipSetDevice(h->device));
    if (rank != root) {
        int rc = own_blob_storage(h);
        if (rc) return rc;
    }
    IdcNcclId id;
    memcpy(&id, unique_id, sizeof(id));
    void* comm = nullptr;
    int e = r->CommInitRank(&comm, world, id, rank);
    if (e != 0) return fail(&h->err, IDC_ERR_HIP, "ncclCommInitRank failed: %s (%s)", r->GetErrorString ? r->GetErrorString(e) : "?", rccl_where().c_str());
    e = r->Broadcast(h->d_blob, (void*)h->d_blob, h->plan.total_bytes, /*ncclUint8*/ 1, root, comm, h->stream.get());
    hipError_t he = hipStreamSynchronize(h->stream.get());
    (void)r->CommDestroy(comm);
    if (e != 0) return fail(&h->err, IDC_ERR_HIP, "ncclBroadcast failed: %s (%s)", r->GetErrorString ? r->GetErrorString(e) : "?", rccl_where().c_str());
    if (he != hipSuccess) return fail(&h->err, IDC_ERR_HIP, "stream sync after ncclBroadcast: %s", hipGetErrorString(he));
    if (rank != root) {                     // the received bytes are validated like any other device blob
        h->weights_set = false;
        int rc = verify_device_blob(h, h->d_blob, h->plan.total_bytes);
        if (rc) return rc;
        h->weights_set = true;
    }
    return IDC_OK;
}

}  // extern "C"
