//go:build stormck

// Package objectstore: GetObject for many object IDs at once through libstormck (the objects
// call).
//
// objectstore.GetObject (objectstore/objectstore.go:15-38) traces one object ID down to its
// blob leaf and probes that leaf by open addressing (findObject). GetObjectsHost and
// GetObjectsDevice do both stages for n IDs in one call over one object tree of a store image,
// every block on the way verified against the checksum its parent holds, and return the found
// objects in a dense array.
// A storm maintainer adds this file to github.com/outofforest/storm/objectstore; nothing in
// storm changes. These entry points work on a store image (host memory or HBM), not on a
// *cache.Cache, so they exist only under the stormck tag.
//
// The slot layout comes from T itself: object_size is unsafe.Sizeof(T), and the library derives
// unsafe.Sizeof(blob.Object[T]) = (8 + Sizeof(T) + 1 + 7) &^ 7 from it, which holds for every T
// of alignment at most 8 (objectSize checks it against the compiler's own answer).
//
// Not compiled in this repository (no Go toolchain in the build image). The C side it
// binds is exercised by tests/test_objects.py and tests/test_objects_gpu.py.
package objectstore

/*
#cgo CFLAGS: -I${SRCDIR}/../third_party/stormck/include
#cgo LDFLAGS: -L${SRCDIR}/../third_party/stormck/lib -lstormck -Wl,-rpath,${SRCDIR}/../third_party/stormck/lib
#include <stdint.h>
#include "stormck.h"
*/
import "C"

import (
	"unsafe"

	"github.com/pkg/errors"

	"github.com/outofforest/storm/blocks"
	"github.com/outofforest/storm/blocks/blob"
	"github.com/outofforest/storm/blocks/pointer"
)

// ObjectResult is stormck_object_result (32 bytes).
type ObjectResult struct {
	ObjectID blocks.ObjectID
	Address  blocks.BlockAddress
	Reminder uint64
	Index    uint32
	Probes   uint16
	Status   uint8
	_        uint8
}

// Statuses of an ObjectResult: the trace's.
const (
	ObjectFound    = uint8(C.STORMCK_TRACE_FOUND)
	ObjectMismatch = uint8(C.STORMCK_TRACE_MISMATCH)
	ObjectRange    = uint8(C.STORMCK_TRACE_RANGE)
	ObjectType     = uint8(C.STORMCK_TRACE_TYPE)
	ObjectAbsent   = uint8(C.STORMCK_TRACE_ABSENT)
	ObjectDepth    = uint8(C.STORMCK_TRACE_DEPTH)
)

// ObjectNoSlot is the Index of an ID whose leaf was not probed, or has no slot left to hand out.
const ObjectNoSlot = uint32(C.STORMCK_LOOKUP_NO_SLOT)

// ObjectStore describes the image one object tree lives in.
type ObjectStore struct {
	Store    unsafe.Pointer // host memory, or a HIP device allocation for GetObjectsDevice
	NBlocks  uint64
	Root     blocks.Pointer
	RootType blocks.BlockType
}

func objectsLayout(s ObjectStore) C.stormck_scrub_layout {
	return C.stormck_scrub_layout{
		block_size:       C.uint64_t(blocks.BlockSize),
		n_blocks:         C.uint64_t(s.NBlocks),
		pointer_fanout:   C.uint32_t(pointer.PointersPerBlock),
		spaces_per_block: 1,
		objectlist_len:   C.uint32_t(blocks.BlockSize),
		blob_len:         C.uint32_t(unsafe.Sizeof(blob.Block{})),
	}
}

// objectSize is unsafe.Sizeof(T), after a check that Go lays blob.Object[T] out as the library
// assumes.
func objectSize[T comparable]() (C.uint32_t, error) {
	var t T
	var slot blob.Object[T]
	size := unsafe.Sizeof(t)
	if size == 0 || unsafe.Sizeof(slot) != (8+size+1+7)&^7 || unsafe.Offsetof(slot.Object) != 8 ||
		unsafe.Offsetof(slot.State) != 8+size {
		return 0, errors.Errorf("blob.Object[%T] has a layout the library does not read", t)
	}
	return C.uint32_t(size), nil
}

func objectsError(rc C.int) error {
	if rc == 0 || rc == C.STORMCK_EMISMATCH {
		return nil // a damaged tree is in the results and the report
	}
	return errors.Errorf("stormck error %d: %s", int(rc), C.GoString(C.stormck_last_error()))
}

// GetObjectsHost gets the objects of ids from the object tree of a store image in host memory.
// results[i] is ID i's and objects[i] its object, the zero T when it is not found; the returned
// string is the text of the first bad ID's error ("" when there is none).
func GetObjectsHost[T comparable](s ObjectStore, objectsPerBlock int, ids []blocks.ObjectID, results []ObjectResult,
	objects []T, verifyLeaves bool) (C.stormck_objects_report, string, error) {
	var report C.stormck_objects_report
	n := uint64(len(ids))
	if n == 0 {
		return report, "", nil
	}
	if uint64(len(results)) < n || uint64(len(objects)) < n {
		return report, "", errors.New("results and objects must hold one entry per ID")
	}
	size, err := objectSize[T]()
	if err != nil {
		return report, "", err
	}
	layout := objectsLayout(s)
	root := C.stormck_pointer{checksum: C.uint64_t(s.Root.Checksum), address: C.uint64_t(s.Root.Address),
		birth_revision: C.uint64_t(s.Root.BirthRevision)}
	params := C.stormck_blob_params{objects_per_block: C.uint32_t(objectsPerBlock), object_size: size}
	flags := C.uint32_t(0)
	if !verifyLeaves {
		flags = C.STORMCK_TRACE_LEAVES_UNVERIFIED
	}
	rc := C.stormck_objects_host(s.Store, &layout, &root, C.uint8_t(s.RootType), &params, unsafe.Pointer(&ids[0]), 8,
		C.uint64_t(n), flags, (*C.stormck_object_result)(unsafe.Pointer(&results[0])), unsafe.Pointer(&objects[0]),
		C.uint64_t(size), &report, 0)
	if err := objectsError(rc); err != nil {
		return report, "", err
	}
	if rc != 0 {
		return report, C.GoString(C.stormck_last_error()), nil
	}
	return report, "", nil
}

// GetObjectsDevice is the same over an image, IDs, results and rows that are HIP device
// allocations (s.Store, dIDs, dResults, dObjects), queued on stream (a hipStream_t, nil for the
// default stream); it returns when the results and the rows are written. ID i is the uint64 at
// dIDs + i*idStride: 8 for a dense array, 32 for the results of keystore.GetObjectIDsDevice read
// in place. Row i is unsafe.Sizeof(T) bytes at dObjects + i*Sizeof(T). dWorkspace holds at least
// ObjectsWorkspaceBytes(n) bytes.
func GetObjectsDevice[T comparable](s ObjectStore, objectsPerBlock int, dIDs unsafe.Pointer, idStride uint64, n uint64,
	dResults, dObjects, dWorkspace unsafe.Pointer, workspaceBytes uint64, verifyLeaves bool,
	stream unsafe.Pointer) (C.stormck_objects_report, string, error) {
	var report C.stormck_objects_report
	size, err := objectSize[T]()
	if err != nil {
		return report, "", err
	}
	layout := objectsLayout(s)
	root := C.stormck_pointer{checksum: C.uint64_t(s.Root.Checksum), address: C.uint64_t(s.Root.Address),
		birth_revision: C.uint64_t(s.Root.BirthRevision)}
	params := C.stormck_blob_params{objects_per_block: C.uint32_t(objectsPerBlock), object_size: size}
	flags := C.uint32_t(0)
	if !verifyLeaves {
		flags = C.STORMCK_TRACE_LEAVES_UNVERIFIED
	}
	rc := C.stormck_objects_device(s.Store, &layout, &root, C.uint8_t(s.RootType), &params, dIDs, C.uint64_t(idStride),
		C.uint64_t(n), flags, (*C.stormck_object_result)(dResults), dObjects, C.uint64_t(size), dWorkspace,
		C.uint64_t(workspaceBytes), &report, stream)
	if err := objectsError(rc); err != nil {
		return report, "", err
	}
	if rc != 0 {
		return report, C.GoString(C.stormck_last_error()), nil
	}
	return report, "", nil
}

// ObjectsWorkspaceBytes is the device workspace a call with n IDs needs.
func ObjectsWorkspaceBytes(n uint64) uint64 {
	return uint64(C.stormck_objects_workspace_bytes(C.uint64_t(n)))
}
