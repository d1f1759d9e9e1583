// Launch chain (ercgraft.h): a captured step -- a HIP graph that is one simple path of kernel nodes -- replayed as plain
// hipLaunchKernel calls from C.  Host code only: nothing here runs on the device.
//
// Why: between two replays of an executable graph the queue idles for several microseconds (DESIGN.md findings 48, 64),
// while kernels launched one by one on a stream cross the step boundary like any other kernel boundary.  The graph is still
// what CAPTURES the step (it is the one record of every launch's function, geometry and arguments); only the replay changes.
#include <dlfcn.h>

#include <vector>

#include "erc_common.h"
#include "store_dev.h"

extern "C" int erc_chain_order(int n_nodes, int n_edges, const int32_t* from_host, const int32_t* to_host, int32_t* order_host) {
    ERC_REQUIRE(n_nodes > 0 && order_host != nullptr, "chain_order: n_nodes=%d (need >= 1 and an output array)", n_nodes);
    // a simple path over n nodes has exactly n - 1 edges (this also refuses a duplicated edge of an otherwise good path)
    ERC_REQUIRE(n_edges == n_nodes - 1, "chain_order: %d nodes with %d edges are not one path", n_nodes, n_edges);
    ERC_REQUIRE(n_edges == 0 || (from_host != nullptr && to_host != nullptr), "chain_order: null edge list");
    std::vector<int32_t> next(n_nodes, -1), pred(n_nodes, -1);
    for (int e = 0; e < n_edges; ++e) {
        const int32_t a = from_host[e], b = to_host[e];
        ERC_REQUIRE(a >= 0 && a < n_nodes && b >= 0 && b < n_nodes && a != b, "chain_order: edge %d (%d -> %d) out of range", e, a, b);
        ERC_REQUIRE(next[a] < 0, "chain_order: node %d has two successors (a fork)", a);
        ERC_REQUIRE(pred[b] < 0, "chain_order: node %d has two predecessors (a join)", b);
        next[a] = b;
        pred[b] = a;
    }
    int root = -1, roots = 0;
    for (int i = 0; i < n_nodes; ++i)
        if (pred[i] < 0) {
            root = i;
            ++roots;
        }
    ERC_REQUIRE(roots == 1, "chain_order: %d roots (need exactly one)", roots);
    int len = 0;
    for (int i = root; i >= 0 && len < n_nodes; i = next[i]) order_host[len++] = i;
    // (one root, in- and out-degree <= 1, n - 1 edges: whatever the walk from the root did not reach would be a cycle)
    ERC_REQUIRE(len == n_nodes, "chain_order: only %d of %d nodes hang on the root's path", len, n_nodes);
    return ERC_OK;
}

namespace {

constexpr uint32_t CHAIN_MAGIC = 0x45524343u;      // "ERCC"

struct ChainNode {
    const void* func;
    dim3 grid, block;
    unsigned lds;
    void** params;      // owned by the graph (see ercgraft.h: the chain never outlives it)
};

struct Chain {
    uint32_t magic;
    std::vector<ChainNode> nodes;
};

Chain* chain_of(int64_t handle) {
    Chain* c = reinterpret_cast<Chain*>(static_cast<intptr_t>(handle));
    return (c != nullptr && c->magic == CHAIN_MAGIC) ? c : nullptr;
}

// null + erc_last_error; clears the runtime's sticky last-error so that a refused graph does not fail a later launch check
Chain* refuse(const char* what, hipError_t e) {
    erc_set_error("chain_build: %s%s%s", what, e != hipSuccess ? ": " : "", e != hipSuccess ? hipGetErrorString(e) : "");
    (void)hipGetLastError();
    return nullptr;
}

Chain* build(hipGraph_t graph) {
    if (graph == nullptr) return refuse("null graph", hipSuccess);
    size_t n = 0, n_edges = 0;
    hipError_t e = hipGraphGetNodes(graph, nullptr, &n);
    if (e != hipSuccess) return refuse("hipGraphGetNodes", e);
    if (n == 0 || n > (1u << 20)) return refuse("the graph has no nodes (or too many)", hipSuccess);
    std::vector<hipGraphNode_t> nodes(n);
    if ((e = hipGraphGetNodes(graph, nodes.data(), &n)) != hipSuccess) return refuse("hipGraphGetNodes", e);
    nodes.resize(n);
    if ((e = hipGraphGetEdges(graph, nullptr, nullptr, &n_edges)) != hipSuccess) return refuse("hipGraphGetEdges", e);
    if (n_edges != n - 1) return refuse("the nodes do not form one path (edge count)", hipSuccess);
    std::vector<hipGraphNode_t> from(n_edges + 1), to(n_edges + 1);
    if (n_edges > 0 && (e = hipGraphGetEdges(graph, from.data(), to.data(), &n_edges)) != hipSuccess) return refuse("hipGraphGetEdges", e);
    if (n_edges != n - 1) return refuse("the nodes do not form one path (edge count)", hipSuccess);

    std::vector<ChainNode> found(n);
    for (size_t i = 0; i < n; ++i) {
        hipGraphNodeType type;
        if ((e = hipGraphNodeGetType(nodes[i], &type)) != hipSuccess) return refuse("hipGraphNodeGetType", e);
        if (type != hipGraphNodeTypeKernel) return refuse("a node is not a kernel node (memcpy, memset, host, event ...)", hipSuccess);
        hipKernelNodeParams p;
        if ((e = hipGraphKernelNodeGetParams(nodes[i], &p)) != hipSuccess) return refuse("hipGraphKernelNodeGetParams", e);
        if (p.kernelParams == nullptr || p.extra != nullptr) return refuse("a kernel node passes its arguments through `extra`", hipSuccess);
        // hipLaunchKernel takes the HOST address of a __global__ function; a node recorded from a module launch holds a
        // hipFunction_t instead, which the attribute query below does not know
        hipFuncAttributes attr;
        if ((e = hipFuncGetAttributes(&attr, p.func)) != hipSuccess) return refuse("a kernel node's function cannot be launched by host address", e);
        // only this library's own kernels: everything they read is in their arguments and in device memory.  A framework's
        // captured kernel may depend on state the framework refreshes when IT replays the graph (torch: the Philox offset
        // of a generator used under capture), which a plain launch would silently skip
        Dl_info own, theirs;
        if (dladdr(reinterpret_cast<const void*>(&erc_chain_order), &own) == 0 || dladdr(p.func, &theirs) == 0 ||
            own.dli_fbase != theirs.dli_fbase)
            return refuse("a kernel node's function is not one of libercgraft's kernels", hipSuccess);
        found[i] = ChainNode{p.func, p.gridDim, p.blockDim, p.sharedMemBytes, p.kernelParams};
    }
    // node handles -> indices; the path order comes from the edges
    std::vector<int32_t> fi(n_edges + 1), ti(n_edges + 1), order(n);
    for (size_t k = 0; k < n_edges; ++k) {
        int32_t a = -1, b = -1;
        for (size_t i = 0; i < n; ++i) {
            if (nodes[i] == from[k]) a = (int32_t)i;
            if (nodes[i] == to[k]) b = (int32_t)i;
        }
        fi[k] = a;
        ti[k] = b;
    }
    if (erc_chain_order((int)n, (int)n_edges, fi.data(), ti.data(), order.data()) != ERC_OK) return nullptr;   // (error text set)
    Chain* c = new Chain{CHAIN_MAGIC, {}};
    c->nodes.reserve(n);
    for (size_t i = 0; i < n; ++i) c->nodes.push_back(found[order[i]]);
    return c;
}

}  // namespace

extern "C" int64_t erc_chain_build(void* graph_host) {
    return static_cast<int64_t>(reinterpret_cast<intptr_t>(build(static_cast<hipGraph_t>(graph_host))));
}

extern "C" int erc_chain_len(int64_t chain) {
    Chain* c = chain_of(chain);
    ERC_REQUIRE(c != nullptr, "chain_len: not a chain handle");
    return (int)c->nodes.size();
}

extern "C" int erc_chain_run(int64_t chain, void* stream) {
    Chain* c = chain_of(chain);
    ERC_REQUIRE(c != nullptr, "chain_run: not a chain handle");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n = c->nodes.size();
    for (size_t i = 0; i < n; ++i) {
        const ChainNode& k = c->nodes[i];
        const hipError_t e = hipLaunchKernel(k.func, k.grid, k.block, k.params, k.lds, s);
        if (e != hipSuccess) {
            erc_set_error("chain_run: launch %d of %d failed: %s", (int)i, (int)n, hipGetErrorString(e));
            (void)hipGetLastError();
            return ERC_E_LAUNCH;
        }
    }
    return ERC_OK;
}

extern "C" int erc_chain_free(int64_t chain) {
    if (chain == 0) return ERC_OK;
    Chain* c = chain_of(chain);
    ERC_REQUIRE(c != nullptr, "chain_free: not a chain handle");
    c->magic = 0;
    delete c;
    return ERC_OK;
}

// ---- store mode of the step's output stores (csrc/store_dev.h): process-wide, read by the launching entry points when they
//      fill a kernel's parameter struct -- so a captured launch keeps the mode it was captured with
static int g_store_mode = 1;
int erc_store_mode(void) { return g_store_mode; }
extern "C" int erc_set_store_mode(int mode) {
    ERC_REQUIRE(mode == 0 || mode == 1, "set_store_mode: mode = %d (0 plain, 1 write-through)", mode);
    g_store_mode = mode;
    return ERC_OK;
}
