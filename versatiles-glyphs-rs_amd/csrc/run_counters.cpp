// run_counters.cpp — run counters of a context and their reduction over the contexts of a run.
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "device_internal.h"

// ---------------------------------------------------------------------------------------
// Run counters and their reduction over the contexts of a run (the one collective of the path —
// results need no exchange, every glyph is independent).  One process drives N devices, one context each; with
// distinct devices the sum is an RCCL all-reduce of 3 x u64 over a communicator of those devices (ncclCommInitAll;
// the library is loaded at first use with dlopen, so libvgsdf.so carries no link-time dependency on RCCL and shares
// the copy a host such as PyTorch has already mapped).  Contexts that share a device (a rehearsal of N lanes on one
// GPU) cannot form a communicator — RCCL refuses two ranks on one device — and are summed on the host.
// ---------------------------------------------------------------------------------------
extern "C" {

namespace {
struct Rccl {
	void *lib = nullptr;
	int (*CommInitAll)(void **, int, const int *) = nullptr;
	int (*CommDestroy)(void *) = nullptr;
	int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
	int (*GroupStart)() = nullptr;
	int (*GroupEnd)() = nullptr;
	const char *(*GetErrorString)(int) = nullptr;
	std::string err;
	bool load()
	{
		if (lib)
			return true;
		for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
			lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
			if (lib)
				break;
		}
		if (!lib) {
			const char *why = dlerror(); // (one call: it clears the message)
			err = std::string("RCCL is not loadable (") + (why ? why : "librccl.so.1") + ")";
			return false;
		}
		auto sym = [&](const char *n) { return dlsym(lib, n); };
		CommInitAll = (decltype(CommInitAll))sym("ncclCommInitAll");
		CommDestroy = (decltype(CommDestroy))sym("ncclCommDestroy");
		AllReduce = (decltype(AllReduce))sym("ncclAllReduce");
		GroupStart = (decltype(GroupStart))sym("ncclGroupStart");
		GroupEnd = (decltype(GroupEnd))sym("ncclGroupEnd");
		GetErrorString = (decltype(GetErrorString))sym("ncclGetErrorString");
		if (!CommInitAll || !CommDestroy || !AllReduce || !GroupStart || !GroupEnd || !GetErrorString) {
			err = "RCCL: a collective entry point is missing from the library";
			dlclose(lib);
			lib = nullptr;
			return false;
		}
		return true;
	}
};
Rccl g_rccl;
// communicators by device list (creating one costs ~100 ms): kept for the life of the process
struct CommSet {
	std::vector<int> devices;
	std::vector<void *> comms;
};
std::vector<CommSet> g_comm_sets;
std::mutex g_comm_mu;
constexpr int kNcclUint64 = 5, kNcclSum = 0; // rccl.h: ncclDataType_t / ncclRedOp_t
} // namespace

void vgsdf_add_counters(vgsdf_ctx *ctx, uint64_t blocks, uint64_t glyphs, uint64_t pixels)
{
	if (!ctx)
		return;
	ctx->counters[0] += blocks;
	ctx->counters[1] += glyphs;
	ctx->counters[2] += pixels;
}

void vgsdf_reset_counters(vgsdf_ctx *ctx)
{
	if (ctx)
		ctx->counters[0] = ctx->counters[1] = ctx->counters[2] = 0;
}

namespace {
// the all-reduce proper: contexts on n DISTINCT devices (n >= 1).  VGSDF_OK: every rank holds `want` (checked)
int reduce_over_rccl(vgsdf_ctx **ctxs, int n, const std::vector<int> &devs, const uint64_t want[3])
{
	vgsdf_ctx *c0 = ctxs[0];
	std::lock_guard<std::mutex> lock(g_comm_mu);
	const char *no_rccl = std::getenv("VGSDF_NO_RCCL"); // (test switch: behave as if librccl were absent)
	if (no_rccl && no_rccl[0] == '1') {
		c0->err = "vgsdf_reduce_counters: RCCL switched off (VGSDF_NO_RCCL=1)";
		return VGSDF_E_HIP;
	}
	if (!g_rccl.load()) {
		c0->err = "vgsdf_reduce_counters: " + g_rccl.err;
		return VGSDF_E_HIP;
	}
	CommSet *set = nullptr;
	for (CommSet &cs : g_comm_sets)
		if (cs.devices == devs)
			set = &cs;
	if (!set) {
		CommSet cs;
		cs.devices = devs;
		cs.comms.assign((size_t)n, nullptr);
		const int rc = g_rccl.CommInitAll(cs.comms.data(), n, devs.data());
		if (rc != 0) {
			c0->err = std::string("vgsdf_reduce_counters: ncclCommInitAll: ") + g_rccl.GetErrorString(rc);
			return VGSDF_E_HIP;
		}
		g_comm_sets.push_back(std::move(cs));
		set = &g_comm_sets.back();
	}
	for (int i = 0; i < n; i++) {
		vgsdf_ctx *c = ctxs[i];
		HIP_TRY(c0, hipSetDevice(c->device));
		if (!c->d_counters)
			HIP_TRY(c0, hipMalloc((void **)&c->d_counters, 3 * sizeof(uint64_t)));
		HIP_TRY(c0, hipMemcpyAsync(c->d_counters, c->counters, 3 * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
		c->comm = set->comms[(size_t)i];
	}
	int rc = g_rccl.GroupStart();
	for (int i = 0; i < n && rc == 0; i++) {
		vgsdf_ctx *c = ctxs[i];
		(void)hipSetDevice(c->device);
		rc = g_rccl.AllReduce(c->d_counters, c->d_counters, 3, kNcclUint64, kNcclSum, c->comm, c->stream);
	}
	const int rc_end = g_rccl.GroupEnd();
	if (rc == 0)
		rc = rc_end;
	if (rc != 0) {
		c0->err = std::string("vgsdf_reduce_counters: RCCL all-reduce: ") + g_rccl.GetErrorString(rc);
		return VGSDF_E_HIP;
	}
	// every rank holds the sum; all of them are read back and must agree with each other and with the host's own sum
	for (int i = 0; i < n; i++) {
		vgsdf_ctx *c = ctxs[i];
		uint64_t got[3] = {0, 0, 0};
		HIP_TRY(c0, hipSetDevice(c->device));
		HIP_TRY(c0, hipMemcpyAsync(got, c->d_counters, sizeof got, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(c0, hipStreamSynchronize(c->stream));
		if (std::memcmp(got, want, sizeof got) != 0) {
			c0->err = "vgsdf_reduce_counters: the all-reduced counters of rank " + std::to_string(i) + " differ from the sum of the ranks' counters";
			return VGSDF_E_HIP;
		}
	}
	return VGSDF_OK;
}

int reduce_counters(vgsdf_ctx **ctxs, int n, uint64_t counters[3], bool strict)
{
	if (!ctxs || n <= 0 || !counters) {
		if (ctxs && n > 0 && ctxs[0])
			ctxs[0]->err = "vgsdf_reduce_counters: NULL argument";
		return VGSDF_E_ARG;
	}
	for (int i = 0; i < n; i++)
		if (!ctxs[i])
			return VGSDF_E_ARG;
	vgsdf_ctx *c0 = ctxs[0];
	std::vector<int> devs((size_t)n);
	bool distinct = true;
	for (int i = 0; i < n; i++) {
		devs[(size_t)i] = ctxs[i]->device;
		for (int j = 0; j < i; j++)
			distinct = distinct && ctxs[j]->device != ctxs[i]->device;
	}
	uint64_t host_sum[3] = {0, 0, 0};
	for (int i = 0; i < n; i++)
		for (int k = 0; k < 3; k++)
			host_sum[k] += ctxs[i]->counters[k];
	// (test switch: take the RCCL branch although contexts share a device — RCCL refuses the communicator, which is how a
	// one-GPU box exercises the fallback)
	if (const char *e = std::getenv("VGSDF_TEST_ASSUME_DISTINCT"))
		distinct = distinct || e[0] == '1';
	if (!distinct) { // lanes sharing a device: no communicator possible (see above)
		if (strict) {
			c0->err = "vgsdf_reduce_counters_rccl: two contexts share a device (RCCL refuses two ranks on one device)";
			return VGSDF_E_ARG;
		}
		c0->reduce_path = "host: contexts share a device";
	} else if (n == 1 && !strict) {
		c0->reduce_path = "host: one context";
	} else {
		const int rc = reduce_over_rccl(ctxs, n, devs, host_sum);
		if (rc == VGSDF_OK) {
			c0->reduce_path = "rccl";
		} else if (strict) {
			return rc;
		} else {
			// The collective carries 24 bytes the host already holds; losing a finished render to it would be absurd.  The
			// sum is taken on the host and the reason kept, loudly: vgsdf_reduce_path() / bench.py `collectives_fallback`.
			c0->reduce_path = "host: RCCL fallback: " + c0->err;
			std::fprintf(stderr, "[vgsdf] %s -- run counters summed on the host\n", c0->err.c_str());
		}
	}
	std::memcpy(counters, host_sum, sizeof host_sum);
	return VGSDF_OK;
}
} // namespace

int vgsdf_reduce_counters(vgsdf_ctx **ctxs, int n, uint64_t counters[3]) { return reduce_counters(ctxs, n, counters, false); }

int vgsdf_reduce_counters_rccl(vgsdf_ctx **ctxs, int n, uint64_t counters[3]) { return reduce_counters(ctxs, n, counters, true); }

const char *vgsdf_reduce_path(const vgsdf_ctx *ctx) { return ctx ? ctx->reduce_path.c_str() : ""; }

} // extern "C"
