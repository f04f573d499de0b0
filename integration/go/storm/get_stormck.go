//go:build stormck

// Package storm: Get for many keys of one space at once through libstormck (the get call).
//
// storm.Get (storm.go:32-58) is spacestore.GetSpace, keystore.GetObjectID and
// objectstore.GetObject, one after the other, for one key. GetManyHost and GetManyDevice do the
// three stages for n keys of one space in one call over a store image, from its singularity
// block, every block on the way verified against the checksum its parent holds.
// A storm maintainer adds this file to github.com/outofforest/storm; nothing in storm changes.
// These entry points work on a store image (host memory or HBM), not on a *cache.Cache, so they
// exist only under the stormck tag.
//
// The library ships no addressing tables: the binding passes spacelist.AddressingOffsets and
// objectlist.AddressingOffsets with every call. object_size is unsafe.Sizeof(T); the library
// derives the slot layout of blob.Object[T] from it (integration/go/objectstore has the check).
//
// Not compiled in this repository (no Go toolchain in the build image). The C side it
// binds is exercised by tests/test_get.py and tests/test_get_gpu.py.
package storm

/*
#cgo CFLAGS: -I${SRCDIR}/third_party/stormck/include
#cgo LDFLAGS: -L${SRCDIR}/third_party/stormck/lib -lstormck -Wl,-rpath,${SRCDIR}/third_party/stormck/lib
#include <stdint.h>
#include "stormck.h"
*/
import "C"

import (
	"runtime"
	"unsafe"

	"github.com/pkg/errors"

	"github.com/outofforest/storm/blocks"
	"github.com/outofforest/storm/blocks/blob"
	"github.com/outofforest/storm/blocks/objectlist"
	"github.com/outofforest/storm/blocks/pointer"
	"github.com/outofforest/storm/blocks/spacelist"
)

// GetResult is stormck_get_result (32 bytes).
type GetResult struct {
	ObjectID      blocks.ObjectID
	KeyAddress    blocks.BlockAddress
	ObjectAddress blocks.BlockAddress
	Index         uint32
	Stage         uint8
	Status        uint8
	_             uint16
}

// Stages of a GetResult: where the key's walk ended.
const (
	GetStageSpace  = uint8(0)
	GetStageKey    = uint8(1)
	GetStageObject = uint8(2)
)

// Statuses of a GetResult: the trace's, and the lookup's KEY.
const (
	GetFound    = uint8(C.STORMCK_TRACE_FOUND)
	GetMismatch = uint8(C.STORMCK_TRACE_MISMATCH)
	GetRange    = uint8(C.STORMCK_TRACE_RANGE)
	GetType     = uint8(C.STORMCK_TRACE_TYPE)
	GetAbsent   = uint8(C.STORMCK_TRACE_ABSENT)
	GetDepth    = uint8(C.STORMCK_TRACE_DEPTH)
	GetKey      = uint8(C.STORMCK_LOOKUP_KEY)
)

func getLayout(nBlocks uint64) C.stormck_scrub_layout {
	return C.stormck_scrub_layout{
		block_size:       C.uint64_t(blocks.BlockSize),
		n_blocks:         C.uint64_t(nBlocks),
		pointer_fanout:   C.uint32_t(pointer.PointersPerBlock),
		spaces_per_block: C.uint32_t(spacelist.SpacesPerBlock),
		objectlist_len:   C.uint32_t(unsafe.Sizeof(objectlist.Block{})),
		blob_len:         C.uint32_t(unsafe.Sizeof(blob.Block{})),
	}
}

func getParams(pin *runtime.Pinner, objectsPerBlock int, objectSize uintptr) C.stormck_get_params {
	pin.Pin(&spacelist.AddressingOffsets[0])
	pin.Pin(&objectlist.AddressingOffsets[0])
	return C.stormck_get_params{
		space_offsets: (*C.uint16_t)(unsafe.Pointer(&spacelist.AddressingOffsets[0])),
		keys: C.stormck_objectlist_params{
			addressing_offsets: (*C.uint16_t)(unsafe.Pointer(&objectlist.AddressingOffsets[0])),
			chunks_per_block:   C.uint32_t(objectlist.ChunksPerBlock)},
		objects: C.stormck_blob_params{objects_per_block: C.uint32_t(objectsPerBlock), object_size: C.uint32_t(objectSize)},
	}
}

func getError(rc C.int) (string, error) {
	if rc == 0 {
		return "", nil
	}
	if rc == C.STORMCK_EMISMATCH {
		return C.GoString(C.stormck_last_error()), nil // a damaged store or a refused key is in the results and the report
	}
	return "", errors.Errorf("stormck error %d: %s", int(rc), C.GoString(C.stormck_last_error()))
}

// GetManyHost gets the objects of keys (key i is keys[i*stride : i*stride+length]) of space
// spaceID from a store image in host memory of nBlocks blocks. results[i] is key i's and
// objects[i] its object, the zero T where there is none; the returned string is the text of the
// first bad key's error ("" when there is none).
func GetManyHost[T comparable](store unsafe.Pointer, nBlocks uint64, spaceID blocks.SpaceID, objectsPerBlock int,
	keys []byte, stride uint64, length uint32, results []GetResult, objects []T,
	verifyLeaves bool) (C.stormck_get_report, string, error) {
	var report C.stormck_get_report
	n := uint64(len(results))
	if n == 0 {
		return report, "", nil
	}
	if uint64(len(objects)) < n {
		return report, "", errors.New("objects must hold one entry per key")
	}
	var t T
	layout := getLayout(nBlocks)
	var pin runtime.Pinner
	defer pin.Unpin()
	params := getParams(&pin, objectsPerBlock, unsafe.Sizeof(t))
	flags := C.uint32_t(0)
	if !verifyLeaves {
		flags = C.STORMCK_TRACE_LEAVES_UNVERIFIED
	}
	rc := C.stormck_get_host(store, &layout, C.uint64_t(spaceID), &params, unsafe.Pointer(&keys[0]), C.uint64_t(stride), nil,
		nil, C.uint32_t(length), C.uint64_t(n), flags, (*C.stormck_get_result)(unsafe.Pointer(&results[0])),
		unsafe.Pointer(&objects[0]), C.uint64_t(unsafe.Sizeof(t)), &report, 0)
	message, err := getError(rc)
	return report, message, err
}

// GetManyDevice is the same over a store, keys, results and rows that are HIP device allocations,
// queued on stream (a hipStream_t, nil for the default stream); it returns when the results and
// the rows are written. Row i is unsafe.Sizeof(T) bytes at dObjects + i*Sizeof(T). dWorkspace
// holds at least GetWorkspaceBytes(n) bytes.
func GetManyDevice[T comparable](dStore unsafe.Pointer, nBlocks uint64, spaceID blocks.SpaceID, objectsPerBlock int,
	dKeys unsafe.Pointer, stride uint64, length uint32, n uint64, dResults, dObjects, dWorkspace unsafe.Pointer,
	workspaceBytes uint64, verifyLeaves bool, stream unsafe.Pointer) (C.stormck_get_report, string, error) {
	var report C.stormck_get_report
	var t T
	layout := getLayout(nBlocks)
	var pin runtime.Pinner
	defer pin.Unpin()
	params := getParams(&pin, objectsPerBlock, unsafe.Sizeof(t))
	flags := C.uint32_t(0)
	if !verifyLeaves {
		flags = C.STORMCK_TRACE_LEAVES_UNVERIFIED
	}
	rc := C.stormck_get_device(dStore, &layout, C.uint64_t(spaceID), &params, dKeys, C.uint64_t(stride), nil, nil,
		C.uint32_t(length), C.uint64_t(n), flags, (*C.stormck_get_result)(dResults), dObjects,
		C.uint64_t(unsafe.Sizeof(t)), dWorkspace, C.uint64_t(workspaceBytes), &report, stream)
	message, err := getError(rc)
	return report, message, err
}

// GetWorkspaceBytes is the device workspace a call with n keys needs.
func GetWorkspaceBytes(n uint64) uint64 {
	return uint64(C.stormck_get_workspace_bytes(C.uint64_t(n), C.uint32_t(objectlist.ChunksPerBlock)))
}
