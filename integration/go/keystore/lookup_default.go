package keystore

import (
	"github.com/outofforest/storm/blocks"
	"github.com/outofforest/storm/cache"
)

// GetObjectIDs is the batch form of GetObjectID over the cache, one GetObjectID per key
// (keystore/keystore.go:18-45). ids[i] and exists[i] are key i's. It is compiled into every
// build, with or without the stormck tag, and does not use libstormck: the library's batched
// lookup (lookup_stormck.go: GetObjectIDsHost, GetObjectIDsDevice) takes a store image, not a
// cache, has other signatures, and exists only under the tag. A caller that wants the library's
// lookup where it is built and this loop elsewhere chooses between them in a tagged file of its
// own.
func GetObjectIDs(c *cache.Cache, origin cache.BlockOrigin, keys [][]byte) ([]blocks.ObjectID, []bool, error) {
	ids := make([]blocks.ObjectID, len(keys))
	exists := make([]bool, len(keys))
	for i, key := range keys {
		id, ok, err := GetObjectID(c, origin, key)
		if err != nil {
			return nil, nil, err
		}
		ids[i], exists[i] = id, ok
	}
	return ids, exists, nil
}
