//go:build stormck

// Package keystore: GetObjectID for many keys at once through libstormck (the lookup).
//
// keystore.GetObjectID (keystore/keystore.go:18-45) hashes one key, traces its tag down
// to the objectlist leaf and probes that leaf by open addressing. GetObjectIDsHost and
// GetObjectIDsDevice do the three stages for n keys in one call over one key tree of a
// store image, every block on the way verified against the checksum its parent holds.
// A storm maintainer adds this file to github.com/outofforest/storm/keystore; nothing in
// storm changes. These entry points work on a store image (host memory or HBM), not on a
// *cache.Cache, so they exist only under the stormck tag: lookup_default.go holds a different
// function, GetObjectIDs over the cache, for every build, and is no stand-in for these.
//
// The library ships no addressing table: it is rand.New(rand.NewSource(0)).Perm(600) of
// Go's math/rand, so the binding passes objectlist.AddressingOffsets and
// objectlist.ChunksPerBlock with every call.
//
// Not compiled in this repository (no Go toolchain in the build image). The C side it
// binds is exercised by tests/test_lookup.py and tests/test_lookup_gpu.py.
package keystore

/*
#cgo CFLAGS: -I${SRCDIR}/../third_party/stormck/include
#cgo LDFLAGS: -L${SRCDIR}/../third_party/stormck/lib -lstormck -Wl,-rpath,${SRCDIR}/../third_party/stormck/lib
#include <stdint.h>
#include "stormck.h"
*/
import "C"

import (
	"runtime"
	"unsafe"

	"github.com/pkg/errors"

	"github.com/outofforest/storm/blocks"
	"github.com/outofforest/storm/blocks/objectlist"
	"github.com/outofforest/storm/blocks/pointer"
)

// LookupResult is stormck_lookup_result (32 bytes).
type LookupResult struct {
	ObjectID blocks.ObjectID
	Address  blocks.BlockAddress
	Reminder uint64
	Index    uint32
	Probes   uint16
	Status   uint8
	_        uint8
}

// Statuses of a LookupResult: the trace's, and LookupKey.
const (
	LookupFound    = uint8(C.STORMCK_TRACE_FOUND)
	LookupMismatch = uint8(C.STORMCK_TRACE_MISMATCH)
	LookupRange    = uint8(C.STORMCK_TRACE_RANGE)
	LookupType     = uint8(C.STORMCK_TRACE_TYPE)
	LookupAbsent   = uint8(C.STORMCK_TRACE_ABSENT)
	LookupDepth    = uint8(C.STORMCK_TRACE_DEPTH)
	LookupKey      = uint8(C.STORMCK_LOOKUP_KEY)
)

// LookupStore describes the image one key tree lives in.
type LookupStore struct {
	Store    unsafe.Pointer // host memory, or a HIP device allocation for GetObjectIDsDevice
	NBlocks  uint64
	Root     blocks.Pointer
	RootType blocks.BlockType
}

func lookupLayout(s LookupStore) C.stormck_scrub_layout {
	return C.stormck_scrub_layout{
		block_size:       C.uint64_t(blocks.BlockSize),
		n_blocks:         C.uint64_t(s.NBlocks),
		pointer_fanout:   C.uint32_t(pointer.PointersPerBlock),
		spaces_per_block: 1,
		objectlist_len:   C.uint32_t(unsafe.Sizeof(objectlist.Block{})),
		blob_len:         C.uint32_t(blocks.BlockSize),
	}
}

func lookupError(rc C.int) error {
	if rc == 0 || rc == C.STORMCK_EMISMATCH {
		return nil // a damaged tree or a refused key is in the results and the report
	}
	return errors.Errorf("stormck error %d: %s", int(rc), C.GoString(C.stormck_last_error()))
}

// GetObjectIDsHost looks up keys (key i is keys[i*stride : i*stride+length]) in the key
// tree of a store image in host memory. results[i] is key i's; the returned string is the
// text of the first bad key's error ("" when there is none).
func GetObjectIDsHost(s LookupStore, keys []byte, stride uint64, length uint32, results []LookupResult,
	verifyLeaves bool) (C.stormck_lookup_report, string, error) {
	var report C.stormck_lookup_report
	n := uint64(len(results))
	if n == 0 {
		return report, "", nil
	}
	layout := lookupLayout(s)
	root := C.stormck_pointer{checksum: C.uint64_t(s.Root.Checksum), address: C.uint64_t(s.Root.Address),
		birth_revision: C.uint64_t(s.Root.BirthRevision)}
	var pin runtime.Pinner
	pin.Pin(&objectlist.AddressingOffsets[0])
	defer pin.Unpin()
	params := C.stormck_objectlist_params{addressing_offsets: (*C.uint16_t)(unsafe.Pointer(&objectlist.AddressingOffsets[0])),
		chunks_per_block: C.uint32_t(objectlist.ChunksPerBlock)}
	flags := C.uint32_t(0)
	if !verifyLeaves {
		flags = C.STORMCK_TRACE_LEAVES_UNVERIFIED
	}
	rc := C.stormck_lookup_host(s.Store, &layout, &root, C.uint8_t(s.RootType), &params, unsafe.Pointer(&keys[0]),
		C.uint64_t(stride), nil, nil, C.uint32_t(length), C.uint64_t(n), flags,
		(*C.stormck_lookup_result)(unsafe.Pointer(&results[0])), nil, nil, &report, 0)
	if err := lookupError(rc); err != nil {
		return report, "", err
	}
	if rc != 0 {
		return report, C.GoString(C.stormck_last_error()), nil
	}
	return report, "", nil
}

// GetObjectIDsDevice is the same over an image, keys and results that are HIP device
// allocations (s.Store, dKeys, dResults), queued on stream (a hipStream_t, nil for the default
// stream); it returns when the results are written. dWorkspace holds at least
// LookupWorkspaceBytes(n) bytes.
func GetObjectIDsDevice(s LookupStore, dKeys unsafe.Pointer, stride uint64, length uint32, n uint64,
	dResults, dWorkspace unsafe.Pointer, workspaceBytes uint64, verifyLeaves bool,
	stream unsafe.Pointer) (C.stormck_lookup_report, string, error) {
	var report C.stormck_lookup_report
	layout := lookupLayout(s)
	root := C.stormck_pointer{checksum: C.uint64_t(s.Root.Checksum), address: C.uint64_t(s.Root.Address),
		birth_revision: C.uint64_t(s.Root.BirthRevision)}
	var pin runtime.Pinner
	pin.Pin(&objectlist.AddressingOffsets[0])
	defer pin.Unpin()
	params := C.stormck_objectlist_params{addressing_offsets: (*C.uint16_t)(unsafe.Pointer(&objectlist.AddressingOffsets[0])),
		chunks_per_block: C.uint32_t(objectlist.ChunksPerBlock)}
	flags := C.uint32_t(0)
	if !verifyLeaves {
		flags = C.STORMCK_TRACE_LEAVES_UNVERIFIED
	}
	rc := C.stormck_lookup_device(s.Store, &layout, &root, C.uint8_t(s.RootType), &params, dKeys, C.uint64_t(stride),
		nil, nil, C.uint32_t(length), C.uint64_t(n), flags, (*C.stormck_lookup_result)(dResults), nil, nil,
		dWorkspace, C.uint64_t(workspaceBytes), &report, stream)
	if err := lookupError(rc); err != nil {
		return report, "", err
	}
	if rc != 0 {
		return report, C.GoString(C.stormck_last_error()), nil
	}
	return report, "", nil
}

// LookupWorkspaceBytes is the device workspace a lookup of n keys needs.
func LookupWorkspaceBytes(n uint64) uint64 {
	return uint64(C.stormck_lookup_workspace_bytes(C.uint64_t(n), C.uint32_t(objectlist.ChunksPerBlock)))
}
